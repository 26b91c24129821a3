"""CPU: the wide forward convolutions, the 2x2 max pool, the bilinear resize and the whole frozen trunk (csrc/conv2d_wide_kernels.h)
on the emulation build against PyTorch (fp64 = truth, fp32 = yardstick), the plan cache, trunk_served / vgg19_trunk, and the host
validation of the new entry points on the product library.  Widths stay at 32..96: the thread-per-lane emulation takes seconds."""
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import assert_as_accurate_as_fp32_reference
from emul_util import emul_lib  # noqa: F401
import seg_oracle as S

# (N, H, W, Cin, Cout, pool): what each exercises is said where the GPU file reuses them (tests/test_gpu_vgg_features.py)
LAYER_CASES = [
    (1, 5, 7, 3, 32, False),      # the Cin = 3 arm, sizes below one tile
    (2, 14, 14, 32, 64, False),   # 392 positions: no multiple of a tile, the border between two images inside a tile
    (1, 9, 6, 96, 32, True),      # a k-loop of several chunks, odd H, pool with floor
    (1, 18, 22, 64, 96, False),   # more than one block of positions and of channels, channels padded to a tile
]
VARIANTS = [(b, r, cl) for b in (True, False) for r in (True, False) for cl in (False, True)]


def layer_inputs(case, seed=0):
    n, h, w, cin, cout, _ = case
    g = torch.Generator().manual_seed(seed + 131 * cin + cout)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    return x, wt, b


def layer_reference(x, wt, b, relu, pool, dtype):
    y = F.conv2d(x.to(dtype), wt.to(dtype), None if b is None else b.to(dtype), padding=1)
    if relu:
        y = F.relu(y)
    if pool:
        y = F.max_pool2d(y, 2, 2)
    return y.permute(0, 2, 3, 1).contiguous()


def expected_conv_labels(m, cin, cout, tile=0, big_min=512, splitk=0, split_min=512):
    """the arm rule of csrc/conv2d.hip::c2w_plan, restated (knob defaults of csrc/tuning.h)"""
    if cin == 3:
        return ["conv2d_wide cin3"]
    nsteps, ct = 9 * (cin // 32), (cout + 63) // 64
    big = tile == 2 or (tile == 0 and (m + 127) // 128 * ct >= big_min)
    split = splitk
    if split == 0:
        split = 1
        while not big and (m + 63) // 64 * ct * split < split_min and split < 8 and nsteps // (2 * split) >= 9:
            split *= 2
    split = max(1, min(split, nsteps))
    if split > 1:
        return ["conv2d_wide splitk=%d" % split, "conv2d_wide reduce"]
    return ["conv2d_wide t128x64" if big else "conv2d_wide t64x64"]


def run_layer(lib, ops, case, bias, relu, wcl, **knobs):
    """-> (ours [N,h,w,Cout], fp32 yardstick, fp64 truth, trace)"""
    x, wt, b = layer_inputs(case)
    b = b if bias else None
    pool = case[5]
    w_in = wt.contiguous(memory_format=torch.channels_last) if wcl else wt
    lib.launch_trace()
    with lib.tuning(**knobs):
        y = ops.conv2d_wide_forward(x.permute(0, 2, 3, 1).contiguous(), w_in, b, relu=relu, pool=pool)
    return y, layer_reference(x, wt, b, relu, pool, torch.float32), layer_reference(x, wt, b, relu, pool, torch.float64), lib.launch_trace()


@pytest.mark.parametrize("bias,relu,wcl", VARIANTS)
@pytest.mark.parametrize("case", LAYER_CASES, ids=lambda c: "%dx%dx%d_%dto%d%s" % (c[:5] + ("_pool" if c[5] else "",)))
def test_layer_vs_conv2d(emul_lib, case, bias, relu, wcl):
    from mvs_amd import ops
    y, r32, r64, trace = run_layer(emul_lib, ops, case, bias, relu, wcl)
    n, h, w, cin, cout, pool = case
    assert trace == ["conv2d_wide pack"] + expected_conv_labels(n * h * w, cin, cout) + (["pool2x2"] if pool else [])
    assert tuple(y.shape) == tuple(r64.shape) and y.is_contiguous()
    assert_as_accurate_as_fp32_reference(y, r32, r64, what="conv2d_wide %r" % (case,))


@pytest.mark.parametrize("case,knobs,labels", [
    (LAYER_CASES[1], dict(c2w_splitk=3), ["conv2d_wide splitk=3", "conv2d_wide reduce"]),                # three K ranges of three steps
    (LAYER_CASES[2], dict(c2w_splitk=1), ["conv2d_wide t64x64", "pool2x2"]),                             # 27 steps in one range
    (LAYER_CASES[2], dict(c2w_splitk=8), ["conv2d_wide splitk=8", "conv2d_wide reduce", "pool2x2"]),     # 27 steps in ranges of 4: one range is empty
    (LAYER_CASES[3], dict(c2w_tile=2, c2w_splitk=1), ["conv2d_wide t128x64"]),                           # the large tile on 396 positions
])
def test_layer_arms_by_knob(emul_lib, case, knobs, labels):
    """Every arm of the general kernel on a shape the default rule would give another one, the trace asserted; all arms agree
    with the default route within the criterion, and t128x64 / t64x64 to the bit (the accumulation order is the tile's own)."""
    from mvs_amd import ops
    y, r32, r64, trace = run_layer(emul_lib, ops, case, True, True, False, **knobs)
    assert trace == ["conv2d_wide pack"] + labels
    assert_as_accurate_as_fp32_reference(y, r32, r64, what="conv2d_wide %r %r" % (case, knobs))
    if knobs.get("c2w_tile") == 2:
        y64 = run_layer(emul_lib, ops, case, True, True, False, c2w_tile=1, c2w_splitk=1)[0]
        assert torch.equal(y, y64)


@pytest.mark.parametrize("shape,size", [((2, 3, 10, 13), (8, 8)), ((1, 3, 5, 6), (12, 9))])
def test_resize_vs_interpolate(emul_lib, shape, size):
    from mvs_amd import ops
    x = torch.randn(shape, generator=torch.Generator().manual_seed(3))
    emul_lib.launch_trace()
    y = ops.resize_bilinear_cl(x, size)
    assert emul_lib.launch_trace() == ["resize_cl"] and tuple(y.shape) == (shape[0],) + size + (shape[1],) and y.is_contiguous()
    r32 = F.interpolate(x, size=size, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    r64 = F.interpolate(x.double(), size=size, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    assert_as_accurate_as_fp32_reference(y, r32, r64, what="resize %r" % (shape,))


def test_maxpool_odd_sizes(emul_lib):
    from mvs_amd import ops
    x = torch.randn(2, 7, 5, 8, generator=torch.Generator().manual_seed(4))
    emul_lib.launch_trace()
    y = ops.maxpool2x2_cl(x)
    assert emul_lib.launch_trace() == ["pool2x2"]
    assert torch.equal(y, F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1))


def test_forward_only(emul_lib):
    from mvs_amd import ops
    x, wt, b = layer_inputs(LAYER_CASES[0])
    xc = x.permute(0, 2, 3, 1).contiguous()
    with pytest.raises(RuntimeError, match="forward only"):
        ops.conv2d_wide_forward(xc, wt.requires_grad_(True), b)
    with pytest.raises(RuntimeError, match="forward only"):
        ops.resize_bilinear_cl(x.clone().requires_grad_(True), (4, 4))
    with torch.no_grad():
        assert not ops.conv2d_wide_forward(xc, wt, b).requires_grad


# ---- whole trunk --------------------------------------------------------------------------------------------------------
TRUNK_LAYERS = (32, 32, "M", 32, 32, "M", 64, 64, 64, 64, "M", 64, 64, 64, 64, "M", 96, 96, 96, 96)   # VGG19's structure, narrow


def small_trunk(layers=TRUNK_LAYERS, seed=0, bias_scale=0.05):
    from mvs_amd.jdacs.models.seg_dff import conv_trunk
    torch.manual_seed(seed)
    net = conv_trunk(layers)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in net.features:
            if isinstance(m, nn.Conv2d):
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * bias_scale)
    return net.eval()


def plan_args(net):
    from mvs_amd.jdacs.models.seg_dff import trunk_layers
    return [(m.weight, m.bias, relu, pool) for m, relu, pool in trunk_layers(net)]


@pytest.fixture(scope="module")
def trunk_run(emul_lib):
    """the five-block trunk once: (net, x, ours, pack trace, forward trace)"""
    from mvs_amd import ops
    net = small_trunk()
    x = torch.randn(2, 3, 32, 48, generator=torch.Generator().manual_seed(9))
    x_cl = x.permute(0, 2, 3, 1).contiguous()
    ops._TRUNK_PLANS.clear()
    emul_lib.launch_trace()
    plan = ops.trunk_plan(plan_args(net), x_cl.shape, x_cl)
    pack_trace = emul_lib.launch_trace()
    out = ops.conv_trunk_forward(plan, x_cl)
    return net, x, out, pack_trace, emul_lib.launch_trace()


def test_trunk_vs_sequential(trunk_run):
    import copy
    net, x, out, _, _ = trunk_run
    with torch.no_grad():
        r32 = net.features(x).permute(0, 2, 3, 1)
        r64 = copy.deepcopy(net).double().features(x.double()).permute(0, 2, 3, 1)
    assert tuple(out.shape) == (2, 2, 3, 96) and out.is_contiguous()
    assert float(r64.abs().max()) > 0.05      # the comparison is not one of zeros
    assert_as_accurate_as_fp32_reference(out, r32, r64, what="trunk")


def test_trunk_launch_trace(trunk_run):
    """One pack launch per convolution when the plan is made; the forward call launches each layer's arm once, in order."""
    _, _, _, pack_trace, fwd_trace = trunk_run
    assert pack_trace == ["conv2d_wide pack"] * 16
    want, m, cin = [], 2 * 32 * 48, 3
    for v in TRUNK_LAYERS:
        if v == "M":
            want.append("pool2x2")
            m //= 4
        else:
            want += expected_conv_labels(m, cin, v)
            cin = v
    assert fwd_trace == want
    assert want.count("conv2d_wide cin3") == 1 and want.count("pool2x2") == 4 and "conv2d_wide splitk=2" in want and "conv2d_wide t64x64" in want


def test_plan_cache_packs_once_and_follows_new_weights(emul_lib):
    from mvs_amd import ops
    layers = (32, "M", 32)
    net = small_trunk(layers, seed=5)
    x = torch.randn(1, 3, 6, 4, generator=torch.Generator().manual_seed(6))
    x_cl = x.permute(0, 2, 3, 1).contiguous()

    def run():
        emul_lib.launch_trace()
        y = ops.conv_trunk_forward(ops.trunk_plan(plan_args(net), x_cl.shape, x_cl), x_cl)
        return y, emul_lib.launch_trace()

    y0, t0 = run()
    y1, t1 = run()
    assert t0.count("conv2d_wide pack") == 2 and t1.count("conv2d_wide pack") == 0 and t1 == t0[2:]
    assert torch.equal(y0, y1)
    other = small_trunk(layers, seed=77)
    net.load_state_dict(other.state_dict())            # in place: same data_ptr, a new _version
    y2, t2 = run()
    assert t2.count("conv2d_wide pack") == 2
    with torch.no_grad():
        r32, r64 = other.features(x).permute(0, 2, 3, 1), other.double().features(x.double()).permute(0, 2, 3, 1)
    assert_as_accurate_as_fp32_reference(y2, r32, r64, what="after load_state_dict")
    assert float((y2 - y0).abs().max()) > 1e-2
    with torch.no_grad():
        net.features[0].bias.add_(1.0)                 # any in-place edit
    y3, t3 = run()
    assert t3.count("conv2d_wide pack") == 2 and float((y3 - y2).abs().max()) > 1e-2


# ---- trunk_served / vgg19_trunk (no kernel runs) ------------------------------------------------------------------------
def _net(*mods):
    from mvs_amd.jdacs.models.seg_dff import _Trunk
    return _Trunk(nn.Sequential(*mods))


def test_trunk_served():
    from mvs_amd.jdacs.models.seg_dff import trunk_layers, trunk_served, vgg19_trunk
    from mvs_amd.jdacs_ms.models import seg_dff as ms
    assert ms.trunk_served is trunk_served and ms.vgg19_trunk is vgg19_trunk
    vgg = vgg19_trunk()
    assert trunk_served(vgg)
    ls = trunk_layers(vgg)
    assert len(ls) == 16 and all(r for _, r, _ in ls) and [i for i, l in enumerate(ls) if l[2]] == [1, 3, 7, 11]
    assert not trunk_served(S.StandInNet())
    assert not trunk_served(_net(nn.Conv2d(3, 32, 5, padding=2), nn.ReLU()))
    assert not trunk_served(_net(nn.Conv2d(3, 32, 3, padding=1), nn.ReLU(), nn.MaxPool2d(3, 2)))
    assert not trunk_served(_net(nn.Conv2d(3, 48, 3, padding=1), nn.ReLU()))
    assert not trunk_served(_net(nn.Conv2d(3, 32, 3, padding=1), nn.ReLU(), nn.MaxPool2d(2, 2, ceil_mode=True)))
    assert not trunk_served(_net(nn.Conv2d(3, 32, 3, padding=1), nn.MaxPool2d(2, 2)))          # a pool not directly after a ReLU
    assert not trunk_served(_net(nn.Conv2d(3, 32, 3, padding=1, stride=2), nn.ReLU()))
    assert not trunk_served(_net(nn.Conv2d(3, 32, 3, padding=1), nn.ReLU(), nn.Conv2d(64, 32, 3, padding=1)))
    assert not trunk_served(nn.Linear(3, 3))
    ls = trunk_layers(_net(nn.Conv2d(3, 32, 3, padding=1), nn.Conv2d(32, 64, 3, padding=1), nn.ReLU(), nn.MaxPool2d(2, 2)))
    assert [(r, p) for _, r, p in ls] == [(False, False), (True, True)]                        # a convolution without a ReLU is allowed


def test_vgg19_trunk_has_torchvisions_names_and_shapes():
    from mvs_amd.jdacs.models.seg_dff import vgg19_trunk
    torch.manual_seed(0)
    net = vgg19_trunk()
    idx = [0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28, 30, 32, 34]
    widths = [64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512, 512, 512, 512]
    sd = net.state_dict()
    assert set(sd) == {"features.%d.%s" % (i, k) for i in idx for k in ("weight", "bias")} and len(sd) == 32
    cin = 3
    for i, c in zip(idx, widths):
        assert tuple(sd["features.%d.weight" % i].shape) == (c, cin, 3, 3) and tuple(sd["features.%d.bias" % i].shape) == (c,)
        assert isinstance(net.features[i + 1], nn.ReLU) and float(sd["features.%d.bias" % i].abs().max()) == 0.0
        cin = c
    assert len(net.features) == 36 and "36" not in net.features._modules
    assert all(isinstance(net.features[i], nn.MaxPool2d) for i in (4, 9, 18, 27))
    assert not any(p.requires_grad for p in net.parameters())
    # kaiming_normal_(fan_out, relu): std = sqrt(2 / (Cout * 9))
    wt = sd["features.34.weight"]
    assert abs(float(wt.std()) / (2.0 / (512 * 9)) ** 0.5 - 1.0) < 0.02
    # a whole-model state dict (classifier entries, as a VGG19 weight file has them) loads without renaming
    full = {k: torch.full_like(v, 0.5) for k, v in sd.items()}
    full["classifier.0.weight"] = torch.zeros(4, 4)
    assert float(vgg19_trunk(full).features[34].bias[0]) == 0.5
    with pytest.raises(KeyError, match="features.34.bias"):
        vgg19_trunk({k: v for k, v in sd.items() if k != "features.34.bias"})


def test_segdff_import_error_names_vgg19_trunk():
    from mvs_amd.jdacs.models.seg_dff import SegDFF
    try:
        import torchvision  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match=r"vgg19_trunk\(state_dict="):
            SegDFF(4)
    with pytest.raises(ValueError, match="hip_features=True"):
        SegDFF(4, net=S.StandInNet(), hip_features=True)
    assert SegDFF(4, net=S.StandInNet())._hip_route(torch.zeros(1, 2, 3, 8, 8)) is None


# ---- host validation, on the product library ----------------------------------------------------------------------------
def test_error_convention_of_the_new_entry_points():
    from mvs_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.MvsLib()
    null_calls = [
        ("mvs_conv2d_wide_pack_weights", (None, None, 64, 64, 0, None)),
        ("mvs_conv2d_wide_fwd", (None, None, None, None, None, 1, 8, 8, 64, 64, 1, 0, None)),
        ("mvs_maxpool2x2_cl", (None, None, 1, 8, 8, 64, None)),
        ("mvs_resize_bilinear_cl", (None, None, 1, 3, 8, 8, 4, 4, None)),
        ("mvs_conv_trunk_fwd", (1, None, None, None, None, None, None, None, None, 1, 8, 8, None)),
    ]
    for name, args in null_calls:
        with pytest.raises(ValueError, match="null pointer"):
            lib.call(name, *args)
    with pytest.raises(ValueError, match="steps of 32, got 48 -> 64"):
        lib.call("mvs_conv2d_wide_fwd", None, None, None, None, None, 1, 8, 8, 48, 64, 1, 0, None)
    with pytest.raises(ValueError, match="steps of 32, got 64 -> 640"):
        lib.call("mvs_conv2d_wide_pack_weights", None, None, 64, 640, 0, None)
    with pytest.raises(ValueError, match="multiple of 4"):
        lib.call("mvs_maxpool2x2_cl", None, None, 1, 8, 8, 6, None)
    with pytest.raises(ValueError, match="cannot be pooled"):
        lib.call("mvs_conv2d_wide_fwd", None, None, None, None, None, 1, 1, 8, 64, 64, 1, 1, None)
    assert lib.launch_trace() == []
    assert lib.raw("mvs_conv2d_wide_workspace_floats", 1, 8, 8, 48, 64) == -1
    assert lib.raw("mvs_conv2d_wide_workspace_floats", 0, 8, 8, 64, 64) == -1
    assert lib.raw("mvs_conv2d_wide_packed_floats", 48, 64) == -1
    assert lib.raw("mvs_conv2d_wide_packed_floats", 3, 64) == 1 * 2 * 4 * 256
    assert lib.raw("mvs_conv2d_wide_packed_floats", 64, 96) == 18 * 2 * 8 * 256
    # 7 x 14 x 14 positions, 512 -> 512: 176 t64x64 workgroups -> four K ranges; the image in front of a pool + four partial images
    assert lib.raw("mvs_conv2d_wide_workspace_floats", 7, 14, 14, 512, 512) == 1372 * 512 * 5
    assert lib.raw("mvs_conv2d_wide_workspace_floats", 7, 224, 224, 64, 64) == 7 * 224 * 224 * 64
