"""TEST INFRASTRUCTURE: the case table of the size-selected conv3d arms (csrc/conv3d.hip: run_igemm / run_cin1 / run_wgrad pick a
kernel by launch size and by knobs), shared by

  * tests/test_gpu_conv_arms.py -- every case on the MI355X against an fp64 reference, and
  * tests/test_conv_arm_dispatch.py -- the same calls on the emulation library with the kernels' bodies skipped, asserting only
    the launch trace (mvs_launch_trace): the day a dispatch threshold moves, the case that no longer reaches its arm fails there,
    on a machine without a GPU.

A case = one op (forward / input gradient / weight gradient) at one shape; its `variants` are the knob settings under test, each
with the EXACT launch trace it must leave; `base` is the arm the variant replaces (compared on identical inputs: bitwise where the
project claims it, else to 2e-4 x scale).  Inputs follow test_conv3d_family_vs_torch: randn, weights x 0.2, batch 2."""
import collections

import torch
import torch.nn.functional as F

Variant = collections.namedtuple("Variant", "name knobs trace")
Case = collections.namedtuple("Case", "id op cin cout stride transposed dims epilogue variants base bitwise")

PACK = "conv_pack_weights"
FORCE = {"conv_pers_min": 0}


def _pers_variants(nw=8, extra=None, groups=(3, 0)):
    label = "conv_pers nw=%d" % nw
    out = []
    for g in groups:
        knobs = dict(FORCE, conv_pers_groups=g, **(extra or {}))
        out.append(Variant("groups_%d" % g, knobs, [PACK, label]))
    return out


def _case(id, op, cin, cout, stride, transposed, dims, variants, base=None, epilogue=False, bitwise=False):
    return Case(id, op, cin, cout, stride, transposed, dims, epilogue, variants, base, bitwise)


def _base(knobs, trace):
    return Variant("base", knobs, trace)


NO_SMALL = {"conv_small": 0}     # the transposed 16 -> 8 layer takes the W-parity-merged image (and with it the persistent kernel) only
                                 # on full-size tiles: below conv_small_wgs workgroups the auto tiling picks GEOM_TR2_SMALL first

# ---- conv_pers_kernel, forced at small ragged shapes (a few workgroups walk >= 3 tiles each: the double buffer wraps) ----
PERS_FWD = []
for _ep in (False, True):
    _s = "_epilogue" if _ep else ""
    PERS_FWD += [
        _case("fwd_16_16_s1" + _s, "fwd", 16, 16, 1, False, (5, 6, 21), _pers_variants(), _base({"conv_pers": 0}, [PACK, "conv_igemm s1_small"]), _ep, True),
        _case("fwd_8_16_s2" + _s, "fwd", 8, 16, 2, False, (6, 10, 36), _pers_variants(), _base({"conv_pers": 0}, [PACK, "conv_igemm s2_small"]), _ep, True),
        _case("fwdT_16_8_s2" + _s, "fwd", 16, 8, 2, True, (5, 6, 19), _pers_variants(extra=NO_SMALL),
              _base(dict(NO_SMALL, conv_pers=0), [PACK, "conv_igemm tr2_pw"]), _ep, True),
        _case("fwd_8_32_s1" + _s, "fwd", 8, 32, 1, False, (5, 6, 21), _pers_variants(), _base({"conv_pers": 0}, [PACK, "conv_igemm s1_small"]), _ep, True),
    ]

PERS_DGRAD = [      # the "dgrad" rows of test_emul_kernels.PERS_CASES: summand + BatchNorm backward statistics
    _case("dgrad_16_16_s1", "dgrad", 16, 16, 1, False, (4, 6, 20), _pers_variants(), _base({"conv_pers": 0}, [PACK, "conv_igemm s1_small"]), True, True),
    _case("dgradT_16_8_s2", "dgrad", 16, 8, 2, True, (3, 5, 18), _pers_variants(), _base({"conv_pers": 0}, [PACK, "conv_igemm s2_small"]), True, True),
    _case("dgrad_32_8_s1", "dgrad", 32, 8, 1, False, (4, 7, 19), _pers_variants(), _base({"conv_pers": 0}, [PACK, "conv_igemm s1_small"]), True, True),
    _case("dgrad_8_16_s2", "dgrad", 8, 16, 2, False, (10, 12, 38), _pers_variants(extra=NO_SMALL),
          _base(dict(NO_SMALL, conv_pers=0), [PACK, "conv_igemm tr2_pw"]), True, True),
]

# ---- the same kernel picked by the library itself: no knob set.  Every shape is ragged in D, H and W and gives each of the
# 256 (112 KB of LDS) or 512 (75 KB) persistent workgroups at least three tiles ----
_DEF = [Variant("default", {}, [PACK, "conv_pers nw=8"])]
PERS_DEFAULT = [
    _case("default_fwd_16_16_s1", "fwd", 16, 16, 1, False, (17, 38, 116), _DEF, _base({"conv_pers": 0}, [PACK, "conv_igemm s1_small"]), True, True),      # 800 tiles / 256
    _case("default_dgrad_32_8_s1", "dgrad", 32, 8, 1, False, (25, 42, 148), _DEF, _base({"conv_pers": 0}, [PACK, "conv_igemm s1"]), True, True),         # 1540 tiles / 512, two Cout tiles
    _case("default_fwd_8_16_s2", "fwd", 8, 16, 2, False, (25, 75, 167), _DEF, _base({"conv_pers": 0}, [PACK, "conv_igemm s2_small"]), False, True),       # 840 tiles / 256
    _case("default_fwdT_16_8_s2", "fwd", 16, 8, 2, True, (25, 42, 148), _DEF, _base({"conv_pers": 0}, [PACK, "conv_igemm tr2_pw"]), False, True),         # 1540 tiles / 512
]

# ---- the four-wave instantiations (knob conv_pers_nw = 4) ----
PERS_NW4 = [
    _case("nw4_fwd_16_16_s1", "fwd", 16, 16, 1, False, (5, 6, 21), _pers_variants(4, {"conv_pers_nw": 4}, groups=(3,)),
          _base({"conv_pers": 0}, [PACK, "conv_igemm s1_small"]), True, True),
    _case("nw4_dgradT_16_8_s2", "dgrad", 16, 8, 2, True, (3, 5, 18), _pers_variants(4, {"conv_pers_nw": 4}, groups=(3,)),
          _base({"conv_pers": 0}, [PACK, "conv_igemm s2_small"]), True, True),
]

# ---- conv_wgrad_pers_kernel ----
_WP = [Variant("groups_3", dict(FORCE, wgrad_pers=1, conv_pers_groups=3), ["conv_wgrad_pers", "conv_wgrad_reduce narrow"]),
       Variant("groups_0", dict(FORCE, wgrad_pers=1, conv_pers_groups=0), ["conv_wgrad_pers", "conv_wgrad_reduce narrow"])]
_WB = _base({"wgrad_pers": 0}, ["conv_wgrad nbw=1", "conv_wgrad_reduce narrow"])
WGRAD_PERS = [
    _case("wgrad_16_16_s1", "wgrad", 16, 16, 1, False, (5, 6, 21), _WP, _WB),
    _case("wgrad_8_16_s2", "wgrad", 8, 16, 2, False, (6, 10, 36), _WP, _WB),
    _case("wgradT_16_8_s2", "wgrad", 16, 8, 2, True, (3, 5, 18), _WP, _WB),
    _case("wgrad_8_8_s2", "wgrad", 8, 8, 2, False, (4, 8, 20), _WP, _WB),
    # default dispatch: 1120 tiles >= conv_pers_min, 256 workgroups with four or five tiles each
    _case("default_wgrad_8_16_s2", "wgrad", 8, 16, 2, False, (29, 75, 199), [Variant("default", {}, ["conv_wgrad_pers", "conv_wgrad_reduce wide"])],
          _base({"wgrad_pers": 0}, ["conv_wgrad nbw=1", "conv_wgrad_reduce wide"])),
]

# ---- the generic weight-gradient kernel on quarter-size tiles (knob wgrad_small = 3), CG <= 16 (nbw 1) and CG > 16 (nbw 2) ----
WGRAD_SMALL = []
for _cin, _stride, _dims in ((16, 1, (5, 6, 21)), (8, 1, (5, 6, 21)), (8, 2, (6, 10, 36))):
    for _cout, _nbw in ((16, 1), (32, 2)):
        _tiles_wide = "wide" if _stride == 1 else "narrow"      # 36 quarter tiles at stride 1 (> 32 partial images), 24 at stride 2
        WGRAD_SMALL.append(_case("wgrad_small_%d_%d_s%d" % (_cin, _cout, _stride), "wgrad", _cin, _cout, _stride, False, _dims,
                                 [Variant("wgrad_small_3", {"wgrad_small": 3},
                                          ["conv_wgrad (small tiles) nbw=%d" % _nbw, "conv_wgrad_reduce " + _tiles_wide])],
                                 _base({}, ["conv_wgrad nbw=%d" % _nbw, "conv_wgrad_reduce narrow"])))

# ---- the two reductions of the partial images: 54 tiles -> 54 images (wide), knob wgrad_groups = 24 -> 24 images (narrow) ----
WGRAD_REDUCE = [
    _case("wgrad_reduce_16_16_s1", "wgrad", 16, 16, 1, False, (9, 10, 35),
          [Variant("wide", {}, ["conv_wgrad nbw=1", "conv_wgrad_reduce wide"]),
           Variant("narrow", {"wgrad_groups": 24}, ["conv_wgrad nbw=1", "conv_wgrad_reduce narrow"])]),
]

# ---- Cout == 1: the probability layers (bias epilogue); H not a multiple of 4, W not of the 32- / 16-wide tile ----
COUT1 = [
    _case("cout1_8", "fwd1", 8, 1, 1, False, (5, 11, 37),
          [Variant("h4", {"cout1_h4": 1}, ["conv_cout1 h4"]), Variant("plain", {"cout1_h4": 0}, ["conv_cout1 cin=8"])]),
    _case("cout1_16", "fwd1", 16, 1, 1, False, (5, 11, 37), [Variant("plain", {}, ["conv_cout1 cin=16"])]),
]

# ---- their input gradient (direct Cin == 1 kernel) with BatchNorm backward statistics; 4070 voxels: not a multiple of 4 x 256 ----
CIN1 = [
    _case("cin1_%d" % _c, "dgrad", _c, 1, 1, False, (5, 11, 37),
          [Variant("vpt_1", {"cin1_vpt": 1}, [PACK, "conv_cin1 vpt=1"]), Variant("vpt_4", {"cin1_vpt": 5}, [PACK, "conv_cin1 vpt=4"])], None, True)
    for _c in (8, 16)
]

# ---- the auto tiling (conv_small = 1, the library default; test_conv3d_family_vs_torch forces 0 and 2), either side of the
# threshold, layers the persistent kernel does not serve.  Stride 1: conv_small_wgs x 3 = 1152 workgroups.  Stride 2: x 24 = 9216
# workgroups = 4.7 M input voxels at the compiled threshold, a 600 MB fp64 reference: that one case moves the threshold instead
# (conv_small_wgs = 1 -> 24 workgroups against the 48 of this launch) and leaves conv_small on auto ----
AUTO = [
    _case("auto_8_16_s1_below", "fwd", 8, 16, 1, False, (5, 6, 21), [Variant("default", {}, [PACK, "conv_igemm s1_small"])]),
    _case("auto_8_16_s1_above", "fwd", 8, 16, 1, False, (25, 42, 116), [Variant("default", {}, [PACK, "conv_igemm s1"])]),
    _case("auto_16_32_s2_below", "fwd", 16, 32, 2, False, (9, 14, 39), [Variant("default", {}, [PACK, "conv_igemm s2_small"])]),
    _case("auto_16_32_s2_above", "fwd", 16, 32, 2, False, (9, 14, 39), [Variant("threshold_24", {"conv_small_wgs": 1}, [PACK, "conv_igemm s2"])]),
]

# ---- the remaining labelled arms, which have per-kernel GPU tests of their own (test_gpu_parity.py: test_conv_cout8_forms_and_tile_orders,
# test_conv0_weight_gradient_forms_vs_fp64_autograd): here the trace ties each label to the kernel those tests mean ----
C8_CG1 = [
    _case("c8_fwd_32_8_s1", "fwd", 32, 8, 1, False, (5, 6, 21), [Variant("default", {}, ["conv_c8_fwd_bc"])]),
    _case("c8_wgrad_32_8_s1", "wgrad", 32, 8, 1, False, (5, 6, 21),
          [Variant("output_gradient_shifted", {}, ["conv_c8_wgrad_gs", "conv_wgrad_reduce narrow"]),
           Variant("x_shifted", {"wgrad8_gs": 0}, ["conv_c8_wgrad", "conv_wgrad_reduce narrow"])]),
    _case("cg1_wgrad_8_1_s1", "wgrad", 8, 1, 1, False, (5, 11, 37), [Variant("default", {}, ["conv_wgrad_cg1", "conv_wgrad_reduce wide"])]),
]

ALL = PERS_FWD + PERS_DGRAD + PERS_DEFAULT + PERS_NW4 + WGRAD_PERS + WGRAD_SMALL + WGRAD_REDUCE + COUT1 + CIN1 + AUTO + C8_CG1
GENERIC_LABELS = ("conv_igemm", "conv_wgrad nbw", "conv_wgrad (small")     # what a persistent variant's trace must NOT contain


def ids(cases):
    return [c.id for c in cases]


def make_inputs(case, b=2):
    """fp32 CPU tensors of the case (seeded by its geometry, like the family test)"""
    g = torch.Generator().manual_seed(case.cin * 7 + case.cout + 131 * case.stride + sum(case.dims))
    cin, cout = case.cin, case.cout
    x = torch.randn(b, cin, *case.dims, generator=g)
    wshape = (cin, cout, 3, 3, 3) if case.transposed else (cout, cin, 3, 3, 3)
    w = torch.randn(wshape, generator=g) * 0.2
    inp = {"x": x, "w": w}
    yshape = torch.empty(b, cin, *case.dims, device="meta")
    wm = torch.empty(wshape, device="meta")
    yshape = tuple((F.conv_transpose3d(yshape, wm, stride=case.stride, padding=1, output_padding=case.stride - 1) if case.transposed
                    else F.conv3d(yshape, wm, stride=case.stride, padding=1)).shape)
    if case.op == "fwd" and case.epilogue:
        inp["scale"] = 0.5 + 0.5 * torch.rand(cout, generator=g)      # <= 1: the family test's absolute bound holds for the scaled output
        inp["shift"] = torch.randn(cout, generator=g) * 0.3
        inp["skip"] = torch.randn(yshape, generator=g)
    if case.op == "fwd1":
        inp["shift"] = torch.randn(cout, generator=g) * 0.3             # the layer's bias
    if case.op in ("dgrad", "wgrad"):
        inp["gy"] = torch.randn(yshape, generator=g)
    if case.op == "dgrad":
        raw = torch.randn(x.shape, generator=g)
        gamma, beta = 0.5 + torch.rand(cin, generator=g), torch.randn(cin, generator=g) * 0.3
        mean, var = raw.mean(dim=(0, 2, 3, 4)), raw.var(dim=(0, 2, 3, 4), unbiased=False)
        invstd = torch.rsqrt(var + 1e-5)
        inp["raw"] = raw
        inp["stats"] = torch.stack([mean, invstd, gamma * invstd, beta - mean * gamma * invstd]).contiguous()
        if cout != 1:                                                  # (the Cin == 1 kernel takes no summand)
            inp["add"] = torch.randn(x.shape, generator=g)
        del inp["x"]
        inp["x_shape"] = tuple(x.shape)
    return inp


def _conv(case, x, w):
    if case.transposed:
        return F.conv_transpose3d(x, w, stride=case.stride, padding=1, output_padding=case.stride - 1)
    return F.conv3d(x, w, stride=case.stride, padding=1)


def reference(case, inp, dtype):
    """The op + its epilogue written out in torch on the CPU in `dtype` -> {"out": tensor, "stats": [2, C] or None}."""
    c = lambda t: t.to(dtype)
    w = c(inp["w"])
    if case.op in ("fwd", "fwd1"):
        raw = _conv(case, c(inp["x"]), w)
        stats = None
        if case.op == "fwd":
            stats = torch.stack([raw.sum(dim=(0, 2, 3, 4)), (raw * raw).sum(dim=(0, 2, 3, 4))])
        y = raw
        view = lambda v: c(v).view(1, -1, 1, 1, 1)
        if "scale" in inp:
            y = torch.relu(y * view(inp["scale"]) + view(inp["shift"])) + c(inp["skip"])
        elif "shift" in inp:
            y = y + view(inp["shift"])
        return {"out": y, "stats": stats}
    if case.op == "wgrad":
        wl = torch.zeros_like(w).requires_grad_(True)
        _conv(case, c(inp["x"]), wl).backward(c(inp["gy"]))
        return {"out": wl.grad, "stats": None}
    xl = torch.zeros(inp["x_shape"], dtype=dtype).requires_grad_(True)
    (gx,) = torch.autograd.grad(_conv(case, xl, w), xl, c(inp["gy"]))
    if "add" in inp:
        gx = gx + c(inp["add"])
    raw32, st = inp["raw"], inp["stats"]
    v32 = lambda v: v.view(1, -1, 1, 1, 1)
    active = raw32 * v32(st[2]) + v32(st[3]) > 0            # the ReLU mask exactly as the kernel forms it (fp32, no contraction)
    dyh = gx * active
    xhat = (c(raw32) - c(v32(st[0]))) * c(v32(st[1]))
    return {"out": gx, "stats": torch.stack([dyh.sum(dim=(0, 2, 3, 4)), (dyh * xhat).sum(dim=(0, 2, 3, 4))])}


def run(case, inp, lib):
    """The op through the product's wrappers on the device the tensors of `inp` live on -> {"out", "stats"} (stats: slots summed)."""
    from mvs_amd import ops
    if case.op in ("fwd", "fwd1"):
        y, slots = ops.conv3d_forward(inp["x"], inp["w"], case.stride, case.transposed, scale=inp.get("scale"),
                                      shift=inp.get("shift"), skip=inp.get("skip"), relu="scale" in inp, want_stats=case.op == "fwd")
        return {"out": y, "stats": None if slots is None else slots.sum(0)}
    if case.op == "wgrad":
        return {"out": ops.conv3d_wgrad(inp["x"], inp["gy"], tuple(inp["w"].shape), case.stride, case.transposed), "stats": None}
    dev = inp["gy"].device
    nslots = lib.raw("mvs_bn_slots", case.cin)
    slots = torch.zeros((nslots, 2, case.cin), dtype=torch.float64, device=dev)
    gx = ops.conv3d_dgrad(inp["gy"], inp["w"], inp["x_shape"], case.stride, case.transposed, add=inp.get("add"),
                          bn=(inp["raw"], inp["stats"], slots))
    return {"out": gx, "stats": slots.sum(0)}


def to_device(inp, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items()}
