"""GPU parity tests proper (-m gpu): the HIP path, called through the C ABI, against the oracle.

Small cases: oracle on CPU + committed golden fixtures.  BASELINE config sizes: oracle evaluated with
the same torch ops on the GPU (it is device agnostic) plus size-independent properties (linearity of
the warp, zero variance for identical views, softmax normalisation)."""
import pytest
import torch
import torch.nn.functional as F

from conftest import (assert_as_accurate_as_fp32_reference, assert_grads_as_accurate_as_fp32_reference, calibrate_batchnorm, load_golden,
                      rel_l1, state_dict_from)
import softargmin_cases
from oracle import ref_torch as R

pytestmark = pytest.mark.gpu
# MVS_SKIP_HEAVY=1 (intermediate development runs only): skip the three cases that run the ORACLE's stock torch ops at
# BASELINE's full sizes on the GPU (2-6 minutes each; the HIP path itself takes milliseconds there)
import os
_heavy = pytest.mark.skipif(os.environ.get("MVS_SKIP_HEAVY", "0") == "1", reason="MVS_SKIP_HEAVY=1")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    from mvs_amd import _lib
    _lib._INSTANCE = None
    lib = _lib.get()
    assert lib.raw("mvs_is_emulation") == 0  # the product library, not the test emulation
    return torch.device("cuda:0")


def _cams(b, ns, h, w):
    K, E = R.synthetic_cameras(ns + 1, h, w, 4 * w)
    P = E.clone()
    P[:, :3, :4] = K @ E[:, :3, :4]
    rots, transs = [], []
    for s in range(1, ns + 1):
        r, t = R.relative_projection(P[s:s + 1].repeat(b, 1, 1), P[0:1].repeat(b, 1, 1))
        rots.append(r)
        transs.append(t)
    return torch.stack(rots, 1), torch.stack(transs, 1)


def _param_grads(module, skip=()):
    return {k: p.grad.detach().cpu() for k, p in module.named_parameters() if p.grad is not None and not k.endswith(tuple(skip))}


def _check_param_grads(net, oracle32, oracle64, skip, what):
    """HIP gradients vs the oracle's fp32 gradients, judged against the oracle evaluated in fp64 (conftest criterion)."""
    truth = _param_grads(oracle64, skip)
    return assert_grads_as_accurate_as_fp32_reference(_param_grads(net, skip), _param_grads(oracle32, skip), truth, what=what)


@pytest.mark.parametrize("c,ns,per_pixel,alias,ac,dims", [
    (8, 1, False, False, False, (5, 12, 20)),
    (16, 2, True, True, False, (8, 24, 36)),
    (32, 2, False, False, False, (48, 32, 40)),       # BASELINE config 1 cost volume
    (32, 2, False, False, True, (16, 30, 44)),
    (32, 4, False, False, False, (12, 20, 28)),       # N=5 (config 3 view count)
    (32, 6, False, False, False, (6, 16, 24)),        # N=7 (config 5 view count)
    (16, 5, False, True, False, (6, 16, 24)),         # runtime-NS path
    (32, 3, False, False, False, (10, 19, 27)),       # N=4; ragged tile edges (dead lanes of the backward's pixel blocks)
    (32, 3, True, True, False, (8, 21, 30)),          # per-pixel hypotheses, 3 source views, alias quirk
    (16, 4, True, False, False, (8, 20, 28)),
    (32, 1, False, False, False, (24, 17, 23)),
])
def test_plane_sweep_variance_vs_oracle(dev, c, ns, per_pixel, alias, ac, dims):
    from mvs_amd import ops
    g = torch.Generator().manual_seed(3)
    b = 2
    d, h, w = dims
    rot, trans = _cams(b, ns, h, w)
    ref = torch.randn(b, c, h, w, generator=g)
    srcs = [torch.randn(b, c, h, w, generator=g) for _ in range(ns)]
    if per_pixel:
        depth = 450 + 30 * torch.rand(b, 1, h, w, generator=g) + 20.0 * torch.arange(d).view(1, d, 1, 1)
    else:
        depth = (430 + 9.0 * torch.arange(d)).unsqueeze(0).repeat(b, 1)
    refg = ref.to(dev).requires_grad_(True)
    srcg = [s.to(dev).requires_grad_(True) for s in srcs]
    var = ops.plane_sweep_variance(refg, srcg, rot.to(dev), trans.to(dev), depth.to(dev), align_corners=ac,
                                   ms_alias=alias)
    gup = torch.randn(var.shape, generator=g)
    var.backward(gup.to(dev))
    refc = ref.detach().clone().requires_grad_(True)
    srcc = [s.detach().clone().requires_grad_(True) for s in srcs]
    exp = R.plane_sweep_variance(refc, srcc, [rot[:, i] for i in range(ns)], [trans[:, i] for i in range(ns)], depth,
                                 ms_alias=alias, align_corners=ac)
    exp.backward(gup)
    # the truth of both criteria: the reference's formulas in fp64, forward AND backward (white-noise features with unit
    # variance and steep gradients: the two fp32 chains differ by a few ulp of the sample coordinate, so a blanket bound
    # on |ours - reference| says nothing a per-tensor error ratio against the truth does not say better)
    ref64 = ref.detach().double().requires_grad_(True)
    src64 = [s.detach().double().requires_grad_(True) for s in srcs]
    t64 = R.plane_sweep_variance(ref64, src64, [rot[:, i].double() for i in range(ns)],
                                 [trans[:, i].double() for i in range(ns)], depth.double(), ms_alias=alias, align_corners=ac)
    t64.backward(gup.double())
    assert_as_accurate_as_fp32_reference(var.detach().cpu(), exp.detach(), t64.detach(), what="variance volume")
    names = ["ref"] + ["src%d" % i for i in range(ns)]
    assert_grads_as_accurate_as_fp32_reference(
        {n: a.grad.cpu() for n, a in zip(names, [refg] + srcg)}, {n: t.grad for n, t in zip(names, [refc] + srcc)},
        {n: t.grad for n, t in zip(names, [ref64] + src64)}, what="plane-sweep feature gradients N=%d" % (ns + 1))


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("c,ns,step", [(32, 2, 60.0), (32, 2, 400.0), (16, 3, 150.0), (32, 4, 90.0)])
def test_plane_sweep_backward_wide_depth_range(dev, c, ns, step, variant):
    """Backward with footprints that do not fit one accumulation window: depth segmentation and, for the widest range,
    the global-atomic path for taps outside the window.  variant 0 = per-wave windows, 1 = view-pair kernel (knob)."""
    from mvs_amd import _lib, ops
    lib = _lib.get()
    g = torch.Generator().manual_seed(11)
    b, d, h, w = 1, 40, 26, 38
    rot, trans = _cams(b, ns, h, w)
    ref = torch.randn(b, c, h, w, generator=g)
    srcs = [torch.randn(b, c, h, w, generator=g) for _ in range(ns)]
    depth = (300 + step * torch.arange(d)).unsqueeze(0).repeat(b, 1)
    refg = ref.to(dev).requires_grad_(True)
    srcg = [s.to(dev).requires_grad_(True) for s in srcs]
    # variant 2 = the per-wave-window kernel with its windows switched off (every flush takes the global-atomic path),
    # variant 3 = ... in its 3-waves/SIMD form (one rotating register set for the upstream gradient), variant 4 = ... at ONE
    # wave/SIMD for 3-4 source views, variant 5 = ... with the block lookahead (1-2 source views)
    with lib.tuning(sweep_bwd=1 if variant == 1 else 0, bwd_nowin=1 if variant == 2 else 0, bwd_gd=0 if variant == 3 else 2,
                   bwd_pf=2 if variant == 4 else (1 if variant == 5 else 0)):
        var = ops.plane_sweep_variance(refg, srcg, rot.to(dev), trans.to(dev), depth.to(dev))
        gup = torch.randn(var.shape, generator=g)
        var.backward(gup.to(dev))
        torch.cuda.synchronize()
    refc = ref.clone().requires_grad_(True)
    srcc = [s.clone().requires_grad_(True) for s in srcs]
    exp = R.plane_sweep_variance(refc, srcc, [rot[:, i] for i in range(ns)], [trans[:, i] for i in range(ns)], depth)
    exp.backward(gup)
    for a, t in zip([refg] + srcg, [refc] + srcc):
        assert float((a.grad.cpu() - t.grad).abs().max()) < 2e-3 * max(1.0, float(t.grad.abs().max()))

@pytest.mark.parametrize("c,ns,d,gd", [(32, 2, 131, 2), (16, 1, 130, 2), (32, 2, 129, 0), (8, 4, 70, 2), (32, 2, 130, -1)])
def test_plane_sweep_backward_long_segment(dev, c, ns, d, gd):
    """One depth segment longer than 64 planes with a narrow depth range: the backward stages the per-plane hypotheses 64 planes
    at a time and takes the upstream gradient over in groups of 1 or 2 planes (odd / even tails, refills of the staging row)."""
    from mvs_amd import _lib, ops
    lib = _lib.get()
    g = torch.Generator().manual_seed(5)
    b, h, w = 1, 20, 28
    rot, trans = _cams(b, ns, h, w)
    ref = torch.randn(b, c, h, w, generator=g)
    srcs = [torch.randn(b, c, h, w, generator=g) for _ in range(ns)]
    depth = (430 + 1.5 * torch.arange(d)).unsqueeze(0).repeat(b, 1)
    refg = ref.to(dev).requires_grad_(True)
    srcg = [s.to(dev).requires_grad_(True) for s in srcs]
    with lib.tuning(bwd_gd=max(gd, 0), bwd_pf=1 if gd < 0 else 0, bwd_dslab=d):   # gd = -1: the block-lookahead form
        var = ops.plane_sweep_variance(refg, srcg, rot.to(dev), trans.to(dev), depth.to(dev))
        gup = torch.randn(var.shape, generator=g)
        var.backward(gup.to(dev))
        torch.cuda.synchronize()
    refc = ref.clone().requires_grad_(True)
    srcc = [s.clone().requires_grad_(True) for s in srcs]
    exp = R.plane_sweep_variance(refc, srcc, [rot[:, i] for i in range(ns)], [trans[:, i] for i in range(ns)], depth)
    exp.backward(gup)
    for a, t in zip([refg] + srcg, [refc] + srcc):
        assert float((a.grad.cpu() - t.grad).abs().max()) < 2e-3 * max(1.0, float(t.grad.abs().max()))


@pytest.mark.parametrize("c,ns,d", [(32, 2, 48), (16, 3, 21), (32, 6, 9)])
def test_plane_sweep_fwd_depth_staging_forms_agree(dev, c, ns, d):
    """Knob fwd_dl: 0 = depth loaded per plane, 1 = the slab's per-plane depths staged in LDS (default), 2 = + gathers waited
    for inside the re-gather block.  Same arithmetic: the three volumes are bit-identical (and match the oracle)."""
    from mvs_amd import _lib, ops
    lib = _lib.get()
    g = torch.Generator().manual_seed(9)
    b, h, w = 2, 37, 45
    rot, trans = _cams(b, ns, h, w)
    ref = torch.randn(b, c, h, w, generator=g)
    srcs = [torch.randn(b, c, h, w, generator=g) for _ in range(ns)]
    depth = (430 + 9.0 * torch.arange(d)).unsqueeze(0).repeat(b, 1)
    vols = []
    # (round 6: knob fwd_pt = 1 sends fwd_dl != 0 to the projection-table kernel -- measured slower, off by default; the fourth volume is the cached kernel's dl = 1 form)
    for dl, pt in ((0, 1), (1, 1), (2, 1), (1, 0)):
        with lib.tuning(fwd_dl=dl, fwd_pt=pt), torch.no_grad():
            vols.append(ops.plane_sweep_variance(ref.to(dev), [s.to(dev) for s in srcs], rot.to(dev), trans.to(dev), depth.to(dev)).cpu())
    exp = R.plane_sweep_variance(ref, srcs, [rot[:, i] for i in range(ns)], [trans[:, i] for i in range(ns)], depth)
    assert float((vols[1] - exp).abs().max()) < 2e-4
    assert torch.equal(vols[0], vols[1]) and torch.equal(vols[1], vols[2]) and torch.equal(vols[1], vols[3])


@pytest.mark.parametrize("c,ns,d,hw,per_pixel", [(8, 1, 1, (2, 3), False), (8, 1, 1, (2, 2), True), (16, 2, 2, (3, 2), False),
                                                  (32, 1, 3, (2, 5), False), (32, 4, 1, (5, 3), False)])
def test_plane_sweep_smallest_shapes(dev, c, ns, d, hw, per_pixel):
    """The smallest shapes the C ABI accepts (one depth plane, one source view, images of 2 x 2 ... pixels: tiles, slabs and
    depth segments are all partial), forward and backward."""
    from mvs_amd import ops
    g = torch.Generator().manual_seed(21)
    b = 1
    h, w = hw
    rot, trans = _cams(b, ns, 8, 12)        # cameras of a larger image: sample points fall in and out of the tiny maps
    ref = torch.randn(b, c, h, w, generator=g)
    srcs = [torch.randn(b, c, h, w, generator=g) for _ in range(ns)]
    if per_pixel:
        depth = 450 + 30 * torch.rand(b, d, h, w, generator=g)
    else:
        depth = (430 + 35.0 * torch.arange(d)).unsqueeze(0).repeat(b, 1)
    refg = ref.to(dev).requires_grad_(True)
    srcg = [s.to(dev).requires_grad_(True) for s in srcs]
    var = ops.plane_sweep_variance(refg, srcg, rot.to(dev), trans.to(dev), depth.to(dev))
    gup = torch.randn(var.shape, generator=g)
    var.backward(gup.to(dev))
    refc = ref.clone().requires_grad_(True)
    srcc = [s.clone().requires_grad_(True) for s in srcs]
    exp = R.plane_sweep_variance(refc, srcc, [rot[:, i] for i in range(ns)], [trans[:, i] for i in range(ns)], depth)
    exp.backward(gup)
    assert float((var.detach().cpu() - exp.detach()).abs().max()) < 2e-4
    for a, t in zip([refg] + srcg, [refc] + srcc):
        assert float((a.grad.cpu() - t.grad).abs().max()) < 2e-3 * max(1.0, float(t.grad.abs().max()))


@pytest.mark.parametrize("d,hw,per_pixel", [(1, (1, 1), False), (2, (3, 5), False), (3, (1, 17), True), (5, (2, 9), False), (9, (7, 3), True)])
def test_softargmin_smallest_shapes(dev, d, hw, per_pixel):
    """Soft-argmin + confidence at shapes smaller than one wave's 16 pixels x 4 depth slices (D = 1: the confidence window
    [idx - 1, idx + 2] is clipped on both sides), forward and backward vs the oracle (jdacs/models/module.py:145-151)."""
    from mvs_amd import ops
    gen = torch.Generator().manual_seed(d * 10 + hw[1])
    b = 2
    h, w = hw
    lg = torch.randn(b, d, h, w, generator=gen) * 3
    hyp = 500 + torch.rand(b, d, h, w, generator=gen) * 50 if per_pixel else (425 + 7.0 * torch.arange(d)).unsqueeze(0).repeat(b, 1)
    lgg = lg.to(dev).requires_grad_(True)
    dep, conf = ops.softargmin_conf(lgg, hyp.to(dev))
    gd = torch.randn(dep.shape, generator=gen)
    dep.backward(gd.to(dev))
    lgc = lg.clone().requires_grad_(True)
    e, ec, _ = R.softargmin_conf(lgc, hyp)
    e.backward(gd)
    assert float((dep.detach().cpu() - e.detach()).abs().max()) < 1e-3 and float((conf.cpu() - ec).abs().max()) < 1e-5
    assert float((lgg.grad.cpu() - lgc.grad).abs().max()) < 1e-4 * max(1.0, float(lgc.grad.abs().max()))


@pytest.mark.parametrize("d,hw,per_pixel,seed", softargmin_cases.CASES, ids=softargmin_cases.IDS)
def test_softargmin_depth_count_switches(dev, d, hw, per_pixel, seed):
    """The kernel's size switch on hardware: D = 32 / 33 / 131 / 256 (four lane groups, logits in registers; 33 and 131 leave the
    groups unequal work), D = 257 / 300 (four lane groups re-reading memory), fixed and per-pixel hypotheses, H * W not a multiple
    of a wave's 16 pixels; forward and backward against oracle.ref_torch.softargmin_conf in float64.  No pixel is masked: the
    seeds keep every pixel's E[d] more than 1e-3 from an integer (asserted in softargmin_cases.check)."""
    from mvs_amd import ops
    lg, hyp, gd = softargmin_cases.inputs(d, hw, per_pixel, seed)
    lgg = lg.to(dev).requires_grad_(True)
    dep, conf = ops.softargmin_conf(lgg, hyp.to(dev))
    dep.backward(gd.to(dev))
    softargmin_cases.check(dep.detach().cpu(), conf.cpu(), lgg.grad.cpu(), lg, hyp, gd)


@pytest.mark.parametrize("cin,cout,stride,transposed,dims", [(8, 8, 1, False, (1, 1, 1)), (32, 8, 1, False, (1, 2, 3)),
                                                             (8, 16, 2, False, (2, 2, 2)), (16, 8, 2, True, (1, 1, 1)),
                                                             (16, 16, 1, False, (1, 1, 17)), (8, 1, 1, False, (1, 1, 2)),
                                                             (64, 64, 1, False, (1, 1, 1)), (64, 32, 2, True, (1, 2, 1))])
def test_conv3d_smallest_volumes(dev, cin, cout, stride, transposed, dims):
    """Volumes smaller than one workgroup tile in every dimension (every tile is partial, every tap of some voxels is padding):
    forward, input gradient and weight gradient vs ATen on the CPU (mvsnet.py:40-74 layer shapes)."""
    from mvs_amd import ops
    g = torch.Generator().manual_seed(cin + cout + dims[2])
    x = torch.randn(1, cin, *dims, generator=g, requires_grad=True)
    if transposed:
        w = (torch.randn(cin, cout, 3, 3, 3, generator=g) * 0.2).requires_grad_(True)
        yr = F.conv_transpose3d(x, w, stride=stride, padding=1, output_padding=stride - 1)
    else:
        w = (torch.randn(cout, cin, 3, 3, 3, generator=g) * 0.2).requires_grad_(True)
        yr = F.conv3d(x, w, stride=stride, padding=1)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy)
    with torch.no_grad():
        xg, wg, gyg = x.detach().to(dev), w.detach().to(dev), gy.to(dev)
        y, _ = ops.conv3d_forward(xg, wg, stride, transposed)
        gx = ops.conv3d_dgrad(gyg, wg, tuple(x.shape), stride, transposed)
        gw = ops.conv3d_wgrad(xg, gyg, tuple(w.shape), stride, transposed)
    assert float((y.cpu() - yr).abs().max()) < 2e-4
    assert float((gx.cpu() - x.grad).abs().max()) < 3e-4
    assert float((gw.cpu() - w.grad).abs().max()) < 3e-4 * max(1.0, float(w.grad.abs().max()))


def test_relative_projections_one_launch(dev):
    """mvs_relative_projection (all source views in one launch) vs torch.matmul(src_proj, torch.inverse(ref_proj)) per view
    (jdacs/models/module.py:116-118): at least as close to the fp64 result as the fp32 torch path."""
    from mvs_amd import ops
    K, E = R.synthetic_cameras(5, 128, 160, 640)
    P = E.clone()
    P[:, :3, :4] = K @ E[:, :3, :4]
    ref = torch.stack([P[0], P[2]], 0)
    srcs = [torch.stack([P[1], P[3]], 0), torch.stack([P[4], P[1]], 0), torch.stack([P[3], P[0]], 0)]
    rot, trans = ops.relative_projections([s.to(dev) for s in srcs], ref.to(dev))
    rot, trans = rot.cpu(), trans.cpu()
    for s, sp in enumerate(srcs):
        t64 = sp.double() @ torch.linalg.inv(ref.double())
        e32 = torch.matmul(sp, torch.inverse(ref))
        for got, exp, tru in ((rot[:, s], e32[:, :3, :3], t64[:, :3, :3]), (trans[:, s], e32[:, :3, 3], t64[:, :3, 3])):
            scale = float(tru.abs().max())
            assert float((got.double() - tru).abs().max()) <= max(float((exp.double() - tru).abs().max()), 2e-7 * scale)
            assert float((got - exp).abs().max()) < 1e-5 * scale



def test_cpu_resident_cameras_next_to_gpu_images(dev):
    """proj_matrices left on the CPU while imgs / depth_values are on the GPU (the reference moves every tensor with .cuda() in
    its loop; a caller of the drop-in may not): ops.relative_projections copies the cameras to the feature maps' device and the
    depth map equals the all-GPU call (the earlier host fallback handed a host pointer to the plane-sweep kernel)."""
    from mvs_amd.jdacs.models.mvsnet import MVSNet
    from mvs_amd.synthetic import synthetic_mvsnet_inputs
    torch.manual_seed(2)
    net = MVSNet(refine=False).to(dev).eval()
    imgs, proj, dv = synthetic_mvsnet_inputs(1, 3, 64, 96, 16, seed=5)
    with torch.no_grad():
        a = net(imgs.to(dev), proj.to(dev), dv.to(dev))["depth"]
        b = net(imgs.to(dev), proj, dv.to(dev))["depth"]
    assert b.device == a.device and torch.equal(a, b)
    from mvs_amd import ops
    rot, trans = ops.relative_projections([proj[:, 1], proj[:, 2]], proj[:, 0], like=imgs.to(dev))
    assert rot.device.type == "cuda" and trans.device.type == "cuda"
    with pytest.raises(ValueError):
        ops.relative_projections([proj[:, 1, :3]], proj[:, 0])


def test_golden_homo_warping_and_proj_cost(dev):
    from mvs_amd import ops
    from mvs_amd.jdacs.models.module import homo_warping
    for tag in "ab":
        g = load_golden("g1_homo_warping_" + tag)
        src = g["src_fea"].to(dev).requires_grad_(True)
        # rot/trans from the CPU inverse so the ill-conditioned P_src P_ref^-1 is identical on both sides
        rot, trans = R.relative_projection(g["src_proj"], g["ref_proj"])
        out = ops.HomoWarp.apply(src, rot.to(dev), trans.to(dev), g["depth_values"].to(dev), False)
        with torch.no_grad():
            t64 = R.warp_features(g["src_fea"].double(), rot.double(), trans.double(), g["depth_values"].double())
        assert_as_accurate_as_fp32_reference(out.detach().cpu(), g["out"], t64, what="homo_warping golden " + tag)
        assert float((out.cpu() - g["out"]).abs().max()) < 3e-4
        out.backward(g["grad_out"].to(dev))
        assert float((src.grad.cpu() - g["grad_src"]).abs().max()) < 1e-3
        # public function with on-device inverse (looser: conditioning of the homography, see make_goldens.py)
        out2 = homo_warping(g["src_fea"].to(dev), g["src_proj"].to(dev), g["ref_proj"].to(dev),
                            g["depth_values"].to(dev))
        assert float((out2.cpu() - g["out"]).abs().max()) < 1e-3
    g = load_golden("g3_proj_cost")
    rts = [R.relative_projection(R.ms_projection(g["src_in"][:, s], g["src_ex"][:, s]),
                                 R.ms_projection(g["ref_in"], g["ref_ex"])) for s in range(2)]
    rot = torch.stack([r for r, _ in rts], 1).to(dev)
    trans = torch.stack([t for _, t in rts], 1).to(dev)
    ref = g["ref_fea"].to(dev).requires_grad_(True)
    srcs = [g["src_fea0"].to(dev).requires_grad_(True), g["src_fea1"].to(dev).requires_grad_(True)]
    cost = ops.plane_sweep_variance(ref, srcs, rot, trans, g["hypos"].to(dev), ms_alias=True)
    assert float((cost.cpu() - g["cost"]).abs().max()) < 1e-3 * float(g["cost"].abs().max())
    cost.backward(g["grad_out"].to(dev))
    for a, k in ((ref, "grad_ref"), (srcs[0], "grad_src0"), (srcs[1], "grad_src1")):
        assert float((a.grad.cpu() - g[k]).abs().max()) < 2e-3 * max(1.0, float(g[k].abs().max()))


def test_golden_ms_homo_warping(dev):
    """the jdacs-ms `homo_warping` wrapper itself (jdacs-ms/models/modules.py:62-104) on the GPU against
    the fixtures the imported reference produced: `g3.warped_ms` (forward) and `g3b` (two cases, forward + d/d src)."""
    from mvs_amd.jdacs_ms.models.modules import homo_warping
    g = load_golden("g3_proj_cost")
    w = homo_warping(g["src_fea0"].to(dev), g["ref_in"].to(dev), g["src_in"][:, 0].to(dev), g["ref_ex"].to(dev),
                     g["src_ex"][:, 0].to(dev), g["planes"].to(dev))
    assert float((w.cpu() - g["warped_ms"]).abs().max()) < 1e-3
    g = load_golden("g3b_ms_homo_warping")
    for tag in "ab":
        t = {k[2:]: v for k, v in g.items() if k.startswith(tag + "_")}
        src = t["src"].to(dev).requires_grad_(True)
        w = homo_warping(src, t["ref_in"].to(dev), t["src_in"].to(dev), t["ref_ex"].to(dev), t["src_ex"].to(dev), t["planes"].to(dev))
        assert w.shape == t["warped"].shape
        with torch.no_grad():
            rot, trans = R.relative_projection(R.ms_projection(t["src_in"], t["src_ex"]), R.ms_projection(t["ref_in"], t["ref_ex"]))
            t64 = R.warp_features(t["src"].double(), rot.double(), trans.double(), t["planes"].double())
        # on-device inverse of the ill-conditioned P_src P_ref^-1: loose absolute bound on the values,
        # plus the accuracy criterion with the rotation shared bit-for-bit
        assert float((w.detach().cpu() - t["warped"]).abs().max()) < 1e-3
        from mvs_amd import ops
        w2 = ops.HomoWarp.apply(src, rot.to(dev), trans.to(dev), t["planes"].to(dev), False)
        assert_as_accurate_as_fp32_reference(w2.detach().cpu(), t["warped"], t64, what="ms homo_warping " + tag)
        w.backward(t["grad_out"].to(dev))
        assert float((src.grad.cpu() - t["grad_src"]).abs().max()) < 1e-3 * max(1.0, float(t["grad_src"].abs().max()))


def test_golden_softargmin(dev):
    from mvs_amd import ops
    g = load_golden("g5_softargmin")
    lg = g["logits"].to(dev).requires_grad_(True)
    depth, conf = ops.softargmin_conf(lg, g["depth_values"].to(dev))
    assert float((depth.cpu() - g["depth"]).abs().max()) < 1e-3
    assert float((conf.cpu() - g["conf"]).abs().max()) < 1e-5
    depth.backward(g["grad_depth"].to(dev))
    assert float((lg.grad.cpu() - g["grad_logits"]).abs().max()) < 1e-5 * float(g["grad_logits"].abs().max()) + 1e-5


CONV_CASES = [
    (8, 16, 1, False, (12, 20, 36)), (16, 16, 1, False, (8, 16, 32)), (32, 8, 1, False, (16, 16, 32)),
    (32, 32, 1, False, (6, 8, 20)), (64, 64, 1, False, (3, 4, 20)), (8, 16, 2, False, (8, 16, 40)),
    (16, 32, 2, False, (12, 8, 20)), (32, 64, 2, False, (6, 8, 12)), (64, 32, 2, True, (3, 4, 10)),
    (32, 16, 2, True, (6, 8, 20)), (16, 8, 2, True, (4, 8, 20)), (64, 32, 1, True, (4, 6, 10)),
    (8, 1, 1, False, (8, 10, 34)), (16, 1, 1, False, (4, 6, 18)), (16, 32, 2, False, (5, 7, 9)),
]


@pytest.fixture(params=[0, 2], ids=["full_tiles", "quarter_tiles"])
def conv_tiles(request, dev):
    """The generic implicit-GEMM kernel's two workgroup tilings (knob "conv_small": the library picks by launch size)."""
    from mvs_amd import _lib
    with _lib.get().tuning(conv_small=request.param):
        yield request.param


@pytest.mark.parametrize("cin,cout,stride,transposed,dims", CONV_CASES)
def test_conv3d_family_vs_torch(dev, conv_tiles, cin, cout, stride, transposed, dims):
    """Every conv geometry of both regularisers vs the reference's ATen ops (CPU, fp32)."""
    from mvs_amd import ops
    g = torch.Generator().manual_seed(cin * 7 + cout)
    if transposed or stride == 1 or all(s % 2 == 0 for s in dims):
        pass
    x = torch.randn(2, cin, *dims, generator=g)
    wshape = (cin, cout, 3, 3, 3) if transposed else (cout, cin, 3, 3, 3)
    w = torch.randn(wshape, generator=g) * 0.2
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yr = (F.conv_transpose3d(xr, wr, stride=stride, padding=1, output_padding=stride - 1) if transposed
          else F.conv3d(xr, wr, stride=stride, padding=1))
    y, parts = ops.conv3d_forward(x.to(dev), w.to(dev), stride, transposed, want_stats=True)
    assert float((y.cpu() - yr).abs().max()) < 3e-4
    s = parts.sum(0).float().cpu()
    assert torch.allclose(s[0], yr.detach().sum(dim=(0, 2, 3, 4)), atol=5e-2, rtol=1e-4)
    assert torch.allclose(s[1], (yr.detach() ** 2).sum(dim=(0, 2, 3, 4)), atol=5e-2, rtol=1e-4)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy)
    # (the input gradient of a stride-2 convolution is served for even input dims only -- it runs as a transposed convolution that
    #  writes 2 x the output gradient's grid -- and the host rejects odd ones by name: test_gpu_conv_arms.py /
    #  test_conv_arm_dispatch.py::test_conv3d_stride2_input_gradient_rejects_odd_dims)
    if not (stride == 2 and not transposed and any(s % 2 for s in dims)):
        gx = ops.conv3d_dgrad(gy.to(dev), w.to(dev), tuple(x.shape), stride, transposed)
        assert float((gx.cpu() - xr.grad).abs().max()) < 5e-4
    gw = ops.conv3d_wgrad(x.to(dev), gy.to(dev), wshape, stride, transposed)
    assert float((gw.cpu() - wr.grad).abs().max()) < 1e-3 * max(1.0, float(wr.grad.abs().max()))


@pytest.mark.parametrize("b,dims,groups", [(2, (13, 21, 53), 192), (1, (12, 12, 48), 7), (1, (1, 1, 1), 192)],
                         ids=["ragged_batch_2_with_interior_tiles", "seven_persistent_workgroups", "one_voxel"])
def test_conv0_weight_gradient_forms_vs_fp64_autograd(dev, b, dims, groups):
    """conv0's weight gradient (32 -> 8): the output-gradient-shifted kernel with sixteen and eight waves (knob wgrad8_gs = 2 / 1) and the
    4x4x1-MFMA kernel it replaced (0), each against autograd in fp64 under the conftest criterion (the fp32 yardstick is ATen's own
    fp32 weight gradient), and against each other."""
    from mvs_amd import _lib, ops
    lib = _lib.get()
    g = torch.Generator().manual_seed(23)
    x = torch.randn(b, 32, *dims, generator=g)
    gy = torch.randn(b, 8, *dims, generator=g)
    w64 = torch.zeros(8, 32, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv3d(x.double(), w64, padding=1).backward(gy.double())
    w32 = torch.zeros(8, 32, 3, 3, 3, requires_grad=True)
    F.conv3d(x, w32, padding=1).backward(gy)
    got = {}
    for form in (2, 1, 0):
        with lib.tuning(wgrad8_gs=form, wgrad8_groups=groups):
            got[form] = ops.conv3d_wgrad(x.to(dev), gy.to(dev), (8, 32, 3, 3, 3), 1, False).cpu()
    for form, gw in got.items():
        assert_grads_as_accurate_as_fp32_reference({"w": gw}, {"w": w32.grad}, {"w": w64.grad}, what="conv0 weight gradient, wgrad8_gs=%d" % form)
    scale = max(1.0, float(w64.grad.abs().max()))
    assert float((got[2] - got[0]).abs().max()) < 2e-4 * scale and float((got[1] - got[0]).abs().max()) < 2e-4 * scale


def test_conv0_weight_gradient_forms_agree_at_config2_size(dev):
    """The same three kernels on BASELINE config 2's cost volume (1 x 32 x 192 x 128 x 160: 15360 tiles, 60-80 per persistent workgroup)
    with a smooth non-negative X like the variance volume: the forms differ only in the order of a 3.9 M-term sum per element."""
    from mvs_amd import _lib, ops
    lib = _lib.get()
    g = torch.Generator(device=dev).manual_seed(5)
    x = (torch.randn(1, 32, 192, 128, 160, generator=g, device=dev) ** 2 * 0.3).contiguous(memory_format=torch.channels_last_3d)
    gy = (torch.randn(1, 8, 192, 128, 160, generator=g, device=dev) * 1e-3).contiguous(memory_format=torch.channels_last_3d)
    got = {}
    for form in (2, 1, 0):
        with lib.tuning(wgrad8_gs=form):
            got[form] = ops.conv3d_wgrad(x, gy, (8, 32, 3, 3, 3), 1, False).double().cpu()
    # truth of one (ci, co) plane of taps from an fp64 reduction on the GPU: dW[t][ci][co] = sum_p X[p + t - 1][ci] G[p][co]
    xs, gs = x[0, 5].double(), gy[0, 3].double()
    xp = F.pad(xs, (1, 1, 1, 1, 1, 1))
    truth = torch.stack([(xp[kd:kd + 192, kh:kh + 128, kw:kw + 160] * gs).sum() for kd in range(3) for kh in range(3) for kw in range(3)]).cpu()
    ref_err = float((got[0][3, 5].reshape(-1) - truth).abs().sum() / truth.abs().sum())
    for form in (2, 1):
        err = float((got[form][3, 5].reshape(-1) - truth).abs().sum() / truth.abs().sum())
        assert err <= 4.0 * ref_err + 2e-5, (form, err, ref_err)
        rel = float((got[form] - got[0]).abs().sum() / got[0].abs().sum())
        assert rel < 2e-5, (form, rel)


@pytest.mark.parametrize("cin,dims", [(32, (9, 18, 40)), (16, (8, 22, 16)), (8, (5, 4, 33))])
@pytest.mark.parametrize("k8,xcd", [(7, 1), (7, 0), (1, 1), (1, 0)])
def test_conv_cout8_forms_and_tile_orders(dev, cin, dims, k8, xcd):
    """The Cout == 8 stride-1 layer (conv0, mvsnet.py:40 / network.py:47) in both 4x4x1-MFMA forms (k8 = 1: both operands
    through LDS; k8 = 7: weights / output gradient as the broadcast operand) and both tile orders: forward + epilogue + stat partials + wgrad vs ATen."""
    from mvs_amd import _lib, ops
    lib = _lib.get()
    g = torch.Generator().manual_seed(cin + dims[1])
    x = torch.randn(2, cin, *dims, generator=g)
    w = torch.randn(8, cin, 3, 3, 3, generator=g) * 0.2
    xr, wr = x.clone(), w.clone().requires_grad_(True)
    yr = F.conv3d(xr, wr, padding=1)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy)
    yr = yr.detach()
    with lib.tuning(k8=k8, xcd=xcd):
        y, parts = ops.conv3d_forward(x.to(dev), w.to(dev), 1, False, want_stats=True)
        assert float((y.cpu() - yr).abs().max()) < 3e-4
        s = parts.sum(0).float().cpu()
        assert torch.allclose(s[0], yr.sum(dim=(0, 2, 3, 4)), atol=5e-2, rtol=1e-4)
        assert torch.allclose(s[1], (yr ** 2).sum(dim=(0, 2, 3, 4)), atol=5e-2, rtol=1e-4)
        scale = torch.rand(8, generator=g) + 0.5
        shift = torch.randn(8, generator=g)
        skip = torch.randn(yr.shape, generator=g)
        y2, _ = ops.conv3d_forward(x.to(dev), w.to(dev), 1, False, scale=scale.to(dev), shift=shift.to(dev), relu=True,
                                   skip=skip.to(dev))
        ref2 = F.relu(yr * scale.view(1, 8, 1, 1, 1) + shift.view(1, 8, 1, 1, 1)) + skip
        assert float((y2.cpu() - ref2).abs().max()) < 5e-4
        gw = ops.conv3d_wgrad(x.to(dev), gy.to(dev), tuple(w.shape), 1, False)
        assert float((gw.cpu() - wr.grad).abs().max()) < 1e-3 * max(1.0, float(wr.grad.abs().max()))


def _run_regnet_golden(dev, net, g, has_second, oracle_cls):
    net.load_state_dict(state_dict_from(g))
    net = net.to(dev).train()
    x = g["x"].to(dev).requires_grad_(True)
    y = net(x)
    yt = g["y_train"] if g["y_train"].dim() == 5 else g["y_train"].unsqueeze(1)
    assert float((y.cpu() - yt).abs().max()) < 1e-3 * max(1.0, float(yt.abs().max()))
    y.backward(g["grad_out"].view_as(y).to(dev))
    # truth: the oracle's regulariser in fp64 on the same inputs; yardstick: the reference's own fp32 gradients (fixture)
    o64 = oracle_cls()
    o64.load_state_dict({k: v for k, v in state_dict_from(g).items()})
    o64 = o64.double().train()
    x64 = g["x"].double().requires_grad_(True)
    y64 = o64(x64)
    y64.backward(g["grad_out"].view_as(y64).double())
    ours = {"x": x.grad.cpu(), **{k: p.grad.cpu() for k, p in net.named_parameters()}}
    ref32 = {"x": g["grad_x"], **{k: g["grad." + k] for k, _ in net.named_parameters()}}
    truth = {"x": x64.grad, **{k: p.grad for k, p in o64.named_parameters()}}
    assert_grads_as_accurate_as_fp32_reference(ours, ref32, truth, what="regulariser golden")
    assert rel_l1(x.grad.cpu(), g["grad_x"]) < 5e-3
    sd = net.state_dict()
    for k, v in g.items():
        if k.startswith("after1.") and "num_batches" not in k:
            assert torch.allclose(sd[k[7:]].cpu(), v, atol=1e-5, rtol=1e-3), k
        if k.startswith("after1.") and "num_batches" in k:
            assert int(sd[k[7:]]) == int(v)
    if has_second:
        with torch.no_grad():
            net(g["x2"].to(dev))
    net.eval()
    with torch.no_grad():
        ye = net(g["x"].to(dev))
    yev = g["y_eval"] if g["y_eval"].dim() == 5 else g["y_eval"].unsqueeze(1)
    assert float((ye.cpu() - yev).abs().max()) < 1e-3 * max(1.0, float(yev.abs().max()))


@pytest.mark.parametrize("side_pre", [1, 0])
@pytest.mark.parametrize("cin,cout,stride,transposed,dims", [(8, 16, 2, False, (12, 16, 40)), (16, 16, 1, False, (9, 10, 35)), (16, 8, 2, True, (6, 8, 20)),
                                                             (32, 32, 1, False, (5, 6, 33)), (64, 64, 1, False, (4, 4, 18)), (8, 1, 1, False, (9, 11, 37))])
def test_conv3d_dgrad_with_summand_and_batchnorm_backward_statistics(dev, cin, cout, stride, transposed, dims, side_pre):
    """mvs_conv3d_dgrad / mvs_convT3d_dgrad with `add` and `bn_raw` (round 4: the BatchNorm backward statistics of a block summed
    in the epilogue of the input-gradient kernel that completes its output gradient): gx vs ATen, the slots vs the sums written out
    in torch, then mvs_bn_relu_bwd_slots on those slots vs autograd through batch_norm + relu (backward of module.py:35-42)."""
    from mvs_amd import _lib, ops
    g = torch.Generator().manual_seed(cin * 3 + cout + stride)
    b = 2
    x_shape = (b, cin) + tuple(dims)
    wshape = (cin, cout, 3, 3, 3) if transposed else (cout, cin, 3, 3, 3)
    w = torch.randn(wshape, generator=g) * 0.2
    raw = torch.randn(x_shape, generator=g).requires_grad_(True)
    gamma, beta = 0.5 + torch.rand(cin, generator=g), torch.randn(cin, generator=g) * 0.3
    xin = F.relu(F.batch_norm(raw, None, None, gamma, beta, True, 0.1, 1e-5))
    y = F.conv_transpose3d(xin, w, stride=stride, padding=1, output_padding=stride - 1) if transposed else F.conv3d(xin, w, stride=stride, padding=1)
    gy = torch.randn(y.shape, generator=g)
    add = torch.randn(x_shape, generator=g) if cout != 1 else None
    (gxin_ref,) = torch.autograd.grad(y, xin, gy, retain_graph=True)
    gtot = gxin_ref + (add if add is not None else 0)
    (graw_ref,) = torch.autograd.grad(xin, raw, gtot)
    rawd = raw.detach()
    mean, var = rawd.mean(dim=(0, 2, 3, 4)), rawd.var(dim=(0, 2, 3, 4), unbiased=False)
    invstd = torch.rsqrt(var + 1e-5)
    stats = torch.stack([mean, invstd, gamma * invstd, beta - mean * gamma * invstd]).contiguous()
    lib = _lib.get()
    slots = torch.zeros((lib.raw("mvs_bn_slots", cin), 2, cin), dtype=torch.float64, device=dev)
    with lib.tuning(side_pre=side_pre):
        gx = ops.conv3d_dgrad(gy.to(dev), w.to(dev), x_shape, stride, transposed, add=None if add is None else add.to(dev),
                              bn=(rawd.to(dev), stats.to(dev), slots))
    scale_g = max(1.0, float(gtot.abs().max()))
    assert float((gx.cpu() - gtot).abs().max()) < 5e-4 * scale_g
    view = lambda v: v.view(1, cin, 1, 1, 1)
    dyh = gtot * (rawd * view(stats[2]) + view(stats[3]) > 0)
    xhat = (rawd - view(mean)) * view(invstd)
    s = slots.sum(0).float().cpu()
    assert torch.allclose(s[0], dyh.sum(dim=(0, 2, 3, 4)), atol=2e-2, rtol=2e-4)
    assert torch.allclose(s[1], (dyh * xhat).sum(dim=(0, 2, 3, 4)), atol=2e-2, rtol=2e-4)
    draw, dgamma, dbeta = ops.bn_relu_bwd_slots(gx, rawd.to(dev), stats.to(dev), slots, True)
    assert float((draw.cpu() - graw_ref).abs().max()) < 1e-3 * max(1.0, float(graw_ref.abs().max()))
    assert torch.allclose(dbeta.cpu(), dyh.sum(dim=(0, 2, 3, 4)), atol=2e-2, rtol=2e-4)
    assert torch.allclose(dgamma.cpu(), (dyh * xhat).sum(dim=(0, 2, 3, 4)), atol=2e-2, rtol=2e-4)



def test_golden_costregnet_mvs(dev):
    from mvs_amd.jdacs.models.mvsnet import CostRegNet
    _run_regnet_golden(dev, CostRegNet(), load_golden("g4_costregnet_mvs"), True, R.OracleCostRegNet)


def _oracle64_mvsnet(g, loss_fn):
    """fp64 evaluation of the oracle (the pinned restatement of the reference) on the golden's inputs: the truth both fp32
    paths are measured against.  Returns (intermediates, {param: grad})."""
    o = R.OracleMVSNet(refine=False)
    o.load_state_dict(state_dict_from(g))
    o = o.double().train()
    out = o(g["imgs"].double(), g["proj"].double(), g["depth_values"].double(), return_intermediates=True)
    loss_fn(out["depth"]).backward()
    return out, {k: p.grad for k, p in o.named_parameters()}


def test_golden_mvsnet_end_to_end(dev):
    from mvs_amd.jdacs.models.mvsnet import MVSNet
    g = load_golden("g6_mvsnet_e2e")
    net = MVSNet(refine=False)
    net.load_state_dict(state_dict_from(g))
    net = net.to(dev).train()
    cap = {}
    hk = net.cost_regularization.register_forward_hook(lambda m, i, o: cap.update(var=i[0], logits=o))
    out = net(g["imgs"].to(dev), g["proj"].to(dev), g["depth_values"].to(dev))
    wts64 = torch.linspace(0.5, 1.5, out["depth"].numel(), dtype=torch.float64).view_as(out["depth"])
    t64, grads64 = _oracle64_mvsnet(g, lambda depth: (depth * wts64).mean())
    assert float((cap["var"].cpu() - g["train_variance"]).abs().max()) < 2e-4
    # intermediates: the regulariser's logits, as accurate as the reference's own fp32 logits
    logits = cap["logits"].squeeze(1).cpu()
    assert_as_accurate_as_fp32_reference(logits, g["train_logits"].view_as(logits), t64["logits"].detach(), slack=4.0, floor=1e-5,
                                         what="train logits")
    assert rel_l1(logits, g["train_logits"].view_as(logits)) < 1e-3
    assert rel_l1(out["depth"].cpu(), g["train_depth"]) < 1e-3          # BASELINE tolerance: 1e-3 relative L1
    assert float((out["depth"].cpu() - g["train_depth"]).abs().mean()) < 0.5  # abs-depth L1 (mm)
    assert float((out["photometric_confidence"].cpu() - g["train_conf"]).abs().mean()) < 2e-3
    wts = wts64.float().to(dev)
    (out["depth"] * wts).mean().backward()
    names = [k for k, _ in net.named_parameters() if not k.endswith("prob.bias")]   # d softmax / d bias == 0 exactly
    ours = {k: p.grad.cpu() for k, p in net.named_parameters() if k in names}
    assert_grads_as_accurate_as_fp32_reference(ours, {k: g["grad." + k] for k in names}, {k: grads64[k] for k in names},
                                               what="MVSNet end-to-end (g6)")
    sd = net.state_dict()
    for k, v in g.items():
        if k.startswith("cal."):
            sd[k[4:]] = v.to(dev)
    net.load_state_dict(sd)
    net.eval()
    with torch.no_grad():
        oe = net(g["imgs"].to(dev), g["proj"].to(dev), g["depth_values"].to(dev))
    hk.remove()
    el = cap["logits"].squeeze(1).cpu()
    assert rel_l1(el, g["eval_logits"].view_as(el)) < 1e-3
    assert rel_l1(oe["depth"].cpu(), g["eval_depth"]) < 1e-3
    assert float((oe["photometric_confidence"].cpu() - g["eval_conf"]).abs().mean()) < 2e-3


def test_config1_eval_plumbing(dev):
    """BASELINE config 1: MVSNet forward, N=3, 160x128, D=48, eval mode, vs the oracle on CPU."""
    from mvs_amd.jdacs.models.mvsnet import MVSNet
    torch.manual_seed(0)
    net = MVSNet(refine=False)
    with torch.no_grad():
        net.cost_regularization.prob.weight.mul_(50.0)
    oracle = R.OracleMVSNet(refine=False)
    oracle.load_state_dict(net.state_dict())
    imgs, proj, dv = R.synthetic_mvsnet_inputs(1, 3, 128, 160, 48, seed=1)
    # running statistics := batch statistics on both sides (a non-degenerate eval model), then eval
    net = net.to(dev)
    calibrate_batchnorm(net, imgs.to(dev), proj.to(dev), dv.to(dev))
    calibrate_batchnorm(oracle, imgs, proj, dv)
    with torch.no_grad():
        o = net(imgs.to(dev), proj.to(dev), dv.to(dev))
        r = oracle(imgs, proj, dv)
    assert o["depth"].shape == (1, 32, 40) and o["photometric_confidence"].shape == (1, 32, 40)
    assert float(r["depth"].std()) > 2 * float(dv[0, 1] - dv[0, 0])      # the comparison is on a depth map that varies
    assert rel_l1(o["depth"].cpu(), r["depth"]) < 1e-3
    assert float((o["photometric_confidence"].cpu() - r["photometric_confidence"]).abs().mean()) < 5e-3


def test_config2_full_size_properties_and_gpu_oracle(dev):
    """BASELINE config 2 volume (N=3, features 32x128x160, D=192): HIP vs the oracle's torch ops run
    on the GPU, plus size-independent properties."""
    from mvs_amd import ops
    g = torch.Generator().manual_seed(21)
    b, c, d, h, w, ns = 1, 32, 192, 128, 160, 2
    rot, trans = _cams(b, ns, h, w)
    feats = [F.avg_pool2d(torch.randn(b, c, h, w, generator=g), 5, 1, 2) for _ in range(ns + 1)]  # smooth-ish
    depth = (425 + 2.65 * torch.arange(d)).unsqueeze(0)
    fd = [f.to(dev) for f in feats]
    rd, td, dd = rot.to(dev), trans.to(dev), depth.to(dev)
    var = ops.plane_sweep_variance(fd[0], fd[1:], rd, td, dd)
    exp = R.plane_sweep_variance(fd[0], fd[1:], [rd[:, i] for i in range(ns)], [td[:, i] for i in range(ns)], dd)
    assert var.shape == (1, 32, 192, 128, 160)
    assert float((var - exp).abs().max()) < 3e-4 and float((var - exp).abs().mean()) < 1e-6
    del exp
    # property: identical views + identity homography (align_corners=True sampling) -> variance == 0
    eye = torch.eye(3).view(1, 1, 3, 3).repeat(1, ns, 1, 1).to(dev)
    zero = torch.zeros(1, ns, 3, device=dev)
    v0 = ops.plane_sweep_variance(fd[0], [fd[0]] * ns, eye, zero, dd, align_corners=True)
    assert float(v0.abs().max()) < 1e-6
    # property: the warp is linear in the features
    wa = ops.HomoWarp.apply(fd[1], rd[:, 0], td[:, 0], dd, False)
    wb = ops.HomoWarp.apply(fd[2], rd[:, 0], td[:, 0], dd, False)
    wab = ops.HomoWarp.apply(2.0 * fd[1] - 0.5 * fd[2], rd[:, 0], td[:, 0], dd, False)
    assert float((wab - (2.0 * wa - 0.5 * wb)).abs().max()) < 1e-5
    del wa, wb, wab, v0
    # soft-argmin at full size: depth within the hypothesis range, confidence in [0,1], vs GPU oracle
    lg = torch.randn(1, d, h, w, generator=g).to(dev) * 3
    dep, conf = ops.softargmin_conf(lg, dd)
    e_dep, e_conf, _ = R.softargmin_conf(lg, dd)
    assert float(dep.min()) >= 425.0 - 1e-3 and float(dep.max()) <= float(depth.max()) + 1e-3
    assert float(conf.min()) >= 0 and float(conf.max()) <= 1 + 1e-5
    assert float((dep - e_dep).abs().max()) < 1e-2 and float((conf - e_conf).abs().max()) < 1e-4


def _mvsnet_train_step_three_ways(dev, n, ih, iw, nd, seed, dev64):
    """One MVSNet training step (forward, mvsnet_loss, backward) through (a) the HIP path, (b) the oracle's fp32 torch ops on
    the same GPU ("the reference GPU path"), (c) the oracle in fp64 on `dev64` (the truth).  Returns (net, o, oracle32, r,
    oracle64, t)."""
    from mvs_amd.jdacs.models.mvsnet import MVSNet, mvsnet_loss
    torch.manual_seed(0)
    net = MVSNet(refine=False)
    with torch.no_grad():
        net.cost_regularization.prob.weight.mul_(50.0)
    oracle = R.OracleMVSNet(refine=False)
    oracle.load_state_dict(net.state_dict())
    oracle64 = R.OracleMVSNet(refine=False)
    oracle64.load_state_dict(net.state_dict())
    imgs, proj, dv = R.synthetic_mvsnet_inputs(1, n, ih, iw, nd, seed=seed)
    net = net.to(dev).train()
    oracle = oracle.to(dev).train()
    oracle64 = oracle64.double().to(dev64).train()
    cap = {}
    hk = net.cost_regularization.register_forward_hook(lambda m, i, o: cap.update(logits=o.squeeze(1)))
    o = net(imgs.to(dev), proj.to(dev), dv.to(dev))
    hk.remove()
    o["logits"] = cap["logits"]
    r = oracle(imgs.to(dev), proj.to(dev), dv.to(dev), return_intermediates=True)
    t = oracle64(imgs.double().to(dev64), proj.double().to(dev64), dv.double().to(dev64), return_intermediates=True)
    gt = r["depth"].detach() + 3.0
    mask = torch.ones_like(gt)
    mvsnet_loss(o["depth"], gt, mask).backward()
    R.mvsnet_loss(r["depth"], gt, mask).backward()
    R.mvsnet_loss(t["depth"], gt.double().to(dev64), mask.double().to(dev64)).backward()
    return net, o, oracle, r, oracle64, t


def test_config2_train_step_vs_gpu_oracle(dev):
    """MVSNet fwd+bwd at a reduced config-2 aspect (N=3, 256x320, D=96): depth rel-L1 <= 1e-3, logits and parameter
    gradients as accurate as the oracle's fp32 torch ops on the same GPU, both judged against the oracle in fp64 (CPU)."""
    net, o, oracle, r, oracle64, t = _mvsnet_train_step_three_ways(dev, 3, 256, 320, 96, 1, torch.device("cpu"))
    assert rel_l1(o["depth"], r["depth"]) < 1e-3
    assert_as_accurate_as_fp32_reference(o["logits"].detach().cpu(), r["logits"].detach().cpu(), t["logits"].detach(), floor=1e-5,
                                         what="logits (256x320, D=96)")
    _check_param_grads(net, oracle, oracle64, ("prob.bias",), "MVSNet 256x320 D=96")


@pytest.mark.parametrize("b,dims", [(1, (24, 40, 72)), (2, (5, 6, 19))], ids=["interior_tiles", "ragged_batch_2"])
def test_conv0_input_gradient_split_bf16_form_vs_fp64(dev, b, dims):
    """Opt-in knob conv0_x3 (csrc/conv3d_x3.hip: conv0's input gradient, mvsnet.py:40 backward, as six bf16 MFMA products of
    three-term splits of the fp32 operands, fp32 accumulation) against autograd in fp64: at least as accurate as the default
    fp32-MFMA kernel on the same inputs (gradients with a wide dynamic range), and inside 2e-6 of the result's scale everywhere."""
    from mvs_amd import _lib, ops
    lib = _lib.get()
    g = torch.Generator().manual_seed(31)
    w = torch.randn(8, 32, 3, 3, 3, generator=g) * 0.1
    gy = torch.randn(b, 8, *dims, generator=g) * torch.rand(b, 8, *dims, generator=g).pow(4) * 10
    ref = torch.nn.grad.conv3d_input((b, 32, *dims), w.double(), gy.double(), padding=1)
    got = {}
    for knob in (0, 1):
        with lib.tuning(conv0_x3=knob):
            got[knob] = ops.conv3d_dgrad(gy.to(dev), w.to(dev), (b, 32, *dims), 1, False).cpu().double()
    assert not torch.equal(got[0], got[1])
    e = {k: float((v - ref).abs().sum() / ref.abs().sum()) for k, v in got.items()}
    print("conv0 input gradient, relative L1 error against fp64: fp32 MFMA %.3e, split bf16 %.3e" % (e[0], e[1]))
    assert e[1] <= 1.05 * e[0] + 1e-9 and e[1] < 3e-7
    assert float((got[1] - ref).abs().max()) < 2e-6 * float(ref.abs().max())


def test_conv0_input_gradient_split_bf16_form_at_config2_size(dev):
    """... and at BASELINE config 2's size (1 x 192 x 128 x 160, every tile of the persistent walk) against the default kernel, plus
    linearity in the gradient (a size-independent property of the op)."""
    from mvs_amd import _lib, ops
    lib = _lib.get()
    g = torch.Generator().manual_seed(32)
    w = (torch.randn(8, 32, 3, 3, 3, generator=g) * 0.1).to(dev)
    shape = (1, 32, 192, 128, 160)
    ga = torch.randn(1, 8, 192, 128, 160, generator=g).to(dev).contiguous(memory_format=torch.channels_last_3d)
    gb = torch.randn(1, 8, 192, 128, 160, generator=g).to(dev).contiguous(memory_format=torch.channels_last_3d)
    base = ops.conv3d_dgrad(ga, w, shape, 1, False)
    with lib.tuning(conv0_x3=1):
        xa = ops.conv3d_dgrad(ga, w, shape, 1, False)
        xb = ops.conv3d_dgrad(gb, w, shape, 1, False)
        xab = ops.conv3d_dgrad(2.0 * ga - 0.5 * gb, w, shape, 1, False)
    scale = float(base.abs().max())
    assert not torch.equal(base, xa)
    assert float((xa - base).abs().max()) < 2e-6 * scale and rel_l1(xa, base) < 1e-6
    assert float((xab - (2.0 * xa - 0.5 * xb)).abs().max()) < 4e-6 * scale


@pytest.mark.parametrize("b,dims", [(1, (24, 40, 72)), (2, (5, 6, 19))], ids=["interior_columns", "ragged_batch_2_odd_depth"])
def test_conv0_forward_split_bf16_form_vs_fp64(dev, b, dims):
    """Opt-in knob conv0_x3 bit 1: conv0's forward (32 -> 8, the D-marching split-bf16 kernel) with its fused BatchNorm statistics
    against ATen in fp64 (CPU): at least as accurate as the default fp32-MFMA kernel on the same inputs."""
    from mvs_amd import _lib, ops
    lib = _lib.get()
    g = torch.Generator().manual_seed(33)
    w = torch.randn(8, 32, 3, 3, 3, generator=g) * 0.1
    x = torch.randn(b, 32, *dims, generator=g) * torch.rand(b, 32, *dims, generator=g).pow(4) * 10
    ref = F.conv3d(x.double(), w.double(), padding=1)
    got, stats = {}, {}
    for knob in (0, 2):
        with lib.tuning(conv0_x3=knob):
            y, slots = ops.conv3d_forward(x.to(dev), w.to(dev), 1, False, want_stats=True)
            got[knob], stats[knob] = y.cpu().double(), slots.sum(0).cpu()
    assert not torch.equal(got[0], got[2])
    e = {k: float((v - ref).abs().sum() / ref.abs().sum()) for k, v in got.items()}
    print("conv0 forward, relative L1 error against fp64: fp32 MFMA %.3e, split bf16 %.3e" % (e[0], e[2]))
    assert e[2] <= 1.05 * e[0] + 1e-9 and e[2] < 4e-7
    assert float((got[2] - ref).abs().max()) < 3e-6 * float(ref.abs().max())
    assert float(((stats[2][0] - ref.sum((0, 2, 3, 4))).abs() / ref.abs().sum((0, 2, 3, 4))).max()) < 1e-6
    assert float(((stats[2][1] - ref.pow(2).sum((0, 2, 3, 4))).abs() / ref.pow(2).sum((0, 2, 3, 4))).max()) < 1e-6


def test_conv0_forward_split_bf16_form_at_config2_size(dev):
    """... and at BASELINE config 2's size (1 x 32 x 192 x 128 x 160: 160 columns x 16 depth segments) against the default kernel:
    output, statistics, and linearity in the input."""
    from mvs_amd import _lib, ops
    lib = _lib.get()
    g = torch.Generator().manual_seed(34)
    w = (torch.randn(8, 32, 3, 3, 3, generator=g) * 0.1).to(dev)
    xa = torch.randn(1, 32, 192, 128, 160, generator=g).to(dev).contiguous(memory_format=torch.channels_last_3d)
    xb = torch.randn(1, 32, 192, 128, 160, generator=g).to(dev).contiguous(memory_format=torch.channels_last_3d)
    base, s0 = ops.conv3d_forward(xa, w, 1, False, want_stats=True)
    with lib.tuning(conv0_x3=2):
        ya, s1 = ops.conv3d_forward(xa, w, 1, False, want_stats=True)
        yb, _ = ops.conv3d_forward(xb, w, 1, False)
        yab, _ = ops.conv3d_forward(2.0 * xa - 0.5 * xb, w, 1, False)
    scale = float(base.abs().max())
    assert not torch.equal(base, ya)
    assert float((ya - base).abs().max()) < 3e-6 * scale and rel_l1(ya, base) < 1e-6
    assert float((yab - (2.0 * ya - 0.5 * yb)).abs().max()) < 6e-6 * scale
    t0, t1 = s0.sum(0), s1.sum(0)
    l1 = base.double().abs().sum((0, 2, 3, 4))       # (the channel sums of random data nearly cancel: their yardstick is sum |y|)
    assert float(((t1[0] - t0[0]).abs() / l1).max()) < 1e-7 and float(((t1[1] - t0[1]).abs() / t0[1]).max()) < 1e-6


def test_config2_train_step_with_split_bf16_conv0_input_gradient_vs_gpu_oracle(dev):
    """The reduced config-2 training step of test_config2_train_step_vs_gpu_oracle with the opt-in knob on (forward AND input
    gradient of conv0 as split-bf16 products): the same criteria."""
    from mvs_amd import _lib
    lib = _lib.get()
    with lib.tuning(conv0_x3=3):
        net, o, oracle, r, oracle64, t = _mvsnet_train_step_three_ways(dev, 3, 256, 320, 96, 1, torch.device("cpu"))
    assert rel_l1(o["depth"], r["depth"]) < 1e-3
    _check_param_grads(net, oracle, oracle64, ("prob.bias",), "MVSNet 256x320 D=96, conv0_x3=3")


@_heavy
def test_config2_full_size_train_step_vs_gpu_oracle(dev):
    """BASELINE configs[1] at its real size (N=3, 640x512, D=192, fp32): forward AND backward of the whole model against the
    oracle's torch ops on the same GPU (the 409 ms/step "reference GPU path"), with the oracle in fp64 on the GPU as the
    truth for the gradient criterion."""
    net, o, oracle, r, oracle64, t = _mvsnet_train_step_three_ways(dev, 3, 512, 640, 192, 1, dev)
    assert o["depth"].shape == (1, 128, 160)
    assert rel_l1(o["depth"], r["depth"]) < 1e-3                                   # BASELINE tolerance
    assert rel_l1(o["depth"].double(), t["depth"]) < 1e-3
    assert float((o["photometric_confidence"] - r["photometric_confidence"]).abs().mean()) < 2e-3
    assert_as_accurate_as_fp32_reference(o["logits"].detach().cpu(), r["logits"].detach().cpu(), t["logits"].detach().cpu(), floor=1e-5,
                                         what="logits (config 2, full size)")
    rep = _check_param_grads(net, oracle, oracle64, ("prob.bias",), "MVSNet config 2 full size")
    worst = max(rep.items(), key=lambda kv: kv[1][0])
    print("config-2 full-size gradients: worst HIP error %.2e (%s), fp32 torch-ops error there %.2e" % (worst[1][0], worst[0], worst[1][1]))


def test_golden_costregnet_cvp(dev):
    from mvs_amd.jdacs_ms.models.network import CostRegNet
    _run_regnet_golden(dev, CostRegNet(), load_golden("g4_costregnet_cvp"), False, R.OracleCostRegNetMS)


def test_golden_cvpmvsnet_end_to_end(dev):
    """jdacs-ms: 2-level CVP-MVSNet vs the fixture from the imported reference (train-mode BN)."""
    from mvs_amd.jdacs_ms.models import modules as M
    from mvs_amd.jdacs_ms.models.network import CVPMVSNet
    g = load_golden("g7_cvpmvsnet_e2e")
    net = CVPMVSNet(R.cvp_args(nsrc=2, nscale=2, mode="train"))
    net.load_state_dict(state_dict_from(g), strict=False)
    net = net.to(dev).train()
    t = {k: g[k].to(dev) for k in ("ref_img", "src_imgs", "ref_in", "src_in", "ref_ex", "src_ex", "depth_min",
                                   "depth_max")}
    with torch.no_grad():
        out = net(t["ref_img"], t["src_imgs"], t["ref_in"], t["src_in"], t["ref_ex"], t["src_ex"], t["depth_min"],
                  t["depth_max"])
        hyp = M.calDepthHypo(None, g["depth_up"].to(dev), t["ref_in"], t["src_in"], t["ref_ex"], t["src_ex"],
                             None, None, 0)
    assert float((hyp.cpu() - g["hypos0"]).abs().max()) < 1e-3
    assert len(out["depth_est_list"]) == 2 and out["depth_est_list"][0].shape == g["depth0"].shape
    assert rel_l1(out["depth_est_list"][1].cpu(), g["depth1"]) < 1e-3
    assert rel_l1(out["depth_est_list"][0].cpu(), g["depth0"]) < 1e-3
    assert float((out["prob_confidence"].cpu() - g["conf"]).abs().mean()) < 5e-3
    # the pyramid of all views as one batch (default) == one call per view (network.py:100-105), bit for bit
    try:
        CVPMVSNet.batch_views = False
        with torch.no_grad():
            out1 = net(t["ref_img"], t["src_imgs"], t["ref_in"], t["src_in"], t["ref_ex"], t["src_ex"], t["depth_min"], t["depth_max"])
    finally:
        CVPMVSNet.batch_views = True
    for da, db in zip(out["depth_est_list"], out1["depth_est_list"]):
        assert torch.equal(da, db)


@pytest.mark.parametrize("ih,iw,with_grad", [(128, 160, True), pytest.param(864, 1152, False, marks=_heavy)])
def test_cvp_three_level_train_step_vs_gpu_oracle(dev, ih, iw, with_grad):
    """CVP-MVSNet N=5 (nsrc 4), 3 levels, vs the oracle's torch ops on the same GPU: forward + backward (gradient criterion
    against the oracle in fp64) at 128x160, and the forward at BASELINE configs[3]'s real size (final level 1152x864,
    D = (48, 8, 8))."""
    from mvs_amd.jdacs_ms.models.network import CVPMVSNet
    torch.manual_seed(0)
    args = R.cvp_args(nsrc=4, nscale=3, mode="train")
    net = CVPMVSNet(args)
    oracle = R.OracleCVPMVSNet(args)
    oracle.load_state_dict(net.state_dict())
    g = torch.Generator().manual_seed(4)
    # smooth random images (white noise at 1152x864 makes the refinement levels' depth updates ill-conditioned)
    ref_img = F.avg_pool2d(torch.randn(1, 3, ih, iw, generator=g), 5, 1, 2)
    src_imgs = F.avg_pool2d(torch.randn(4, 3, ih, iw, generator=g), 5, 1, 2).unsqueeze(0)
    K, E = R.synthetic_cameras(5, ih, iw, iw)
    ins = [ref_img, src_imgs, K.unsqueeze(0), K.view(1, 1, 3, 3).repeat(1, 4, 1, 1), E[0].unsqueeze(0),
           E[1:].unsqueeze(0), torch.tensor([425.0]), torch.tensor([425.0 + 47 * 13.5])]
    net = net.to(dev).train()
    oracle = oracle.to(dev).train()
    if not with_grad:
        with torch.no_grad():
            o = net(*[t.to(dev) for t in ins])
            r = oracle(*[t.to(dev) for t in ins])
        assert o["depth_est_list"][0].shape == (1, ih, iw)
        for a, b in zip(o["depth_est_list"], r["depth_est_list"]):
            assert rel_l1(a, b) < 1e-3
        return
    o = net(*[t.to(dev) for t in ins])
    r = oracle(*[t.to(dev) for t in ins])
    for a, b in zip(o["depth_est_list"], r["depth_est_list"]):
        assert rel_l1(a, b) < 1e-3
    oracle64 = R.OracleCVPMVSNet(args)
    oracle64.load_state_dict(net.state_dict())
    oracle64 = oracle64.double().train()
    t = oracle64(*[x.double() for x in ins])
    sum(d.mean() for d in o["depth_est_list"]).backward()
    sum(d.mean() for d in r["depth_est_list"]).backward()
    sum(d.mean() for d in t["depth_est_list"]).backward()
    _check_param_grads(net, oracle, oracle64, ("prob0.bias",), "CVP-MVSNet 3 levels N=5")


def test_config3_shape_batch2_five_views_vs_gpu_oracle(dev):
    """BASELINE config 3 shape class: N=5 views, batch 2 per rank (reduced 128x160, D=32): exercises batch > 1 in
    every kernel and the grouped BatchNorm path (5 view groups x 2 samples) against the oracle on the same GPU."""
    from mvs_amd.jdacs.models.mvsnet import MVSNet
    torch.manual_seed(0)
    net = MVSNet(refine=False)
    with torch.no_grad():
        net.cost_regularization.prob.weight.mul_(50.0)
    oracle = R.OracleMVSNet(refine=False)
    oracle.load_state_dict(net.state_dict())
    imgs, proj, dv = R.synthetic_mvsnet_inputs(2, 5, 128, 160, 32, seed=3)
    imgs[1] = imgs[1] * 0.7 + 0.2
    net = net.to(dev).train()
    oracle = oracle.to(dev).train()
    o = net(imgs.to(dev), proj.to(dev), dv.to(dev))
    r = oracle(imgs.to(dev), proj.to(dev), dv.to(dev))
    assert o["depth"].shape == (2, 32, 40)
    assert rel_l1(o["depth"], r["depth"]) < 1e-3
    o["depth"].mean().backward()
    r["depth"].mean().backward()
    oracle64 = R.OracleMVSNet(refine=False)
    oracle64.load_state_dict({k: v.cpu() for k, v in net.state_dict().items() if "running" not in k and "num_batches" not in k},
                             strict=False)
    oracle64 = oracle64.double().train()
    oracle64(imgs.double(), proj.double(), dv.double())["depth"].mean().backward()
    _check_param_grads(net, oracle, oracle64, ("prob.bias",), "MVSNet N=5 batch 2")
    sd, so = net.state_dict(), oracle.state_dict()
    for k in sd:
        if "running" in k:
            assert torch.allclose(sd[k], so[k], atol=1e-4, rtol=1e-3), k
        if "num_batches" in k:
            assert int(sd[k]) == int(so[k]), k


@pytest.mark.parametrize("ih,iw,nd", [(608, 800, 128), pytest.param(1184, 1600, 256, marks=_heavy)])
def test_config5_shape_seven_views_eval(dev, ih, iw, nd):
    """BASELINE configs[4] shape (N=7 views) in fp32 eval mode vs the GPU oracle: at 800x608 D=128 and at the config's real
    size 1600x1184, D=256 (3.9 GB fp32 cost volume resident in HBM, no depth-slab streaming)."""
    from mvs_amd.jdacs.models.mvsnet import MVSNet
    torch.manual_seed(0)
    net = MVSNet(refine=False)
    with torch.no_grad():
        net.cost_regularization.prob.weight.mul_(50.0)
    oracle = R.OracleMVSNet(refine=False)
    oracle.load_state_dict(net.state_dict())
    imgs, proj, dv = R.synthetic_mvsnet_inputs(1, 7, ih, iw, nd, seed=5)
    net = net.to(dev)
    oracle = oracle.to(dev)
    # running statistics := batch statistics, so that the eval pass is not degenerate
    calibrate_batchnorm(net, imgs.to(dev), proj.to(dev), dv.to(dev))
    calibrate_batchnorm(oracle, imgs.to(dev), proj.to(dev), dv.to(dev))
    with torch.no_grad():
        o = net(imgs.to(dev), proj.to(dev), dv.to(dev))
        r = oracle(imgs.to(dev), proj.to(dev), dv.to(dev))
    assert o["depth"].shape == (1, ih // 4, iw // 4)
    assert rel_l1(o["depth"], r["depth"]) < 1e-3
    assert float((o["photometric_confidence"] - r["photometric_confidence"]).abs().mean()) < 5e-3
    del o, r
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", ["g8_unsup_loss", "g8_unsup_loss_n4"])
def test_golden_unsup_loss(dev, name):
    """UnSupLoss through the HIP kernels vs the fixture generated by the imported reference."""
    from mvs_amd.jdacs.losses.unsup_loss import UnSupLoss
    g = load_golden(name)
    depth = g["depth"].to(dev).requires_grad_(True)
    crit = UnSupLoss()
    total = crit(g["imgs"].float().to(dev), g["cams"].to(dev), depth)
    total.backward()
    assert abs(float(total) - float(g["loss"])) < 3e-5 * abs(float(g["loss"]))
    assert abs(float(crit.reconstr_loss) - float(g["reconstr_loss"])) < 2e-5
    assert abs(float(crit.ssim_loss) - float(g["ssim_loss"])) < 2e-5
    assert abs(float(crit.smooth_loss) - float(g["smooth_loss"])) < 2e-4
    gd = g["grad_depth"]
    assert float((depth.grad.cpu() - gd).abs().max()) < 4e-6 + 2e-4 * float(gd.abs().max())


def test_unsup_loss_config3_shape_vs_gpu_oracle(dev):
    """BASELINE config 3 per-GPU shape (N = 5, 640x512 images -> 160x128 loss resolution), batch 2, vs the oracle's
    torch ops on the same GPU; also as the loss of an MVSNet training step (gradient reaches the network)."""
    from mvs_amd.jdacs.losses.unsup_loss import UnSupLoss
    gen = torch.Generator().manual_seed(8)
    b, n, h, w = 2, 5, 512, 640
    imgs = F.avg_pool2d(torch.randn(b * n, 3, h, w, generator=gen), 9, 1, 4).view(b, n, 3, h, w) * 4
    K, E = R.synthetic_cameras(n, h // 4, w // 4, w)
    cams = torch.zeros(b, n, 2, 4, 4)
    cams[:, :, 0] = E
    cams[:, :, 1, :3, :3] = K
    depth = 600.0 + 60.0 * torch.rand(b, h // 4, w // 4, generator=gen)
    imgs, cams = imgs.to(dev), cams.to(dev)
    da, db = depth.to(dev).requires_grad_(True), depth.to(dev).requires_grad_(True)
    la = UnSupLoss()(imgs, cams, da)
    lb = R.unsup_loss(imgs, cams, db)
    la.backward()
    lb.backward()
    assert abs(float(la) - float(lb)) < 3e-5 * abs(float(lb))
    assert float((da.grad - db.grad).abs().max()) < 4e-6 + 3e-4 * float(db.grad.abs().max())
    assert float(da.grad.abs().max()) > 0


def test_config3_self_supervised_step_vs_gpu_oracle(dev):
    """BASELINE config 3 per GPU (N = 5, 640x512, D = 192, one sample): MVSNet forward -> UnSupLoss on its depth map ->
    backward into the network, vs the oracle's MVSNet + UnSupLoss (stock torch ops) on the same GPU and the oracle in fp64.

    The loss has branch points (floor, validity masks, the smooth-L1 knee, top-3 selection): two depth maps that agree to
    1e-6 can still put a pixel on different sides of one.  So the step is checked in two halves that share ONE upstream
    gradient: (a) d loss / d depth of the HIP loss vs the oracle's loss, both evaluated AT THE SAME depth map (element by
    element); (b) that gradient back-propagated through the HIP network, the fp32 oracle and the fp64 oracle: EVERY parameter
    gradient under the fp64-truth criterion used everywhere else (conftest).  (c) The fully independent chains (each path's own
    depth, own loss) are compared by direction / magnitude as before (the worst cosine over ALL parameter tensors is printed)."""
    from mvs_amd.jdacs.losses.unsup_loss import UnSupLoss
    from mvs_amd.jdacs.models.mvsnet import MVSNet
    torch.manual_seed(5)
    net = MVSNet(refine=False)
    with torch.no_grad():
        net.cost_regularization.prob.weight.mul_(50.0)
    oracle = R.OracleMVSNet(refine=False)
    oracle.load_state_dict(net.state_dict())
    oracle64 = R.OracleMVSNet(refine=False)
    oracle64.load_state_dict(net.state_dict())
    net, oracle, oracle64 = net.to(dev).train(), oracle.to(dev).train(), oracle64.double().to(dev).train()
    b, n, h, w, d = 1, 5, 512, 640, 192
    imgs, proj, dv = R.synthetic_mvsnet_inputs(b, n, h, w, d, seed=2)
    imgs = F.avg_pool2d(imgs.view(b * n, 3, h, w), 9, 1, 4).view(b, n, 3, h, w) * 4
    K, E = R.synthetic_cameras(n, h // 4, w // 4, w)
    cams = torch.zeros(b, n, 2, 4, 4)
    cams[:, :, 0] = E
    cams[:, :, 1, :3, :3] = K
    imgs, proj, dv, cams = imgs.to(dev), proj.to(dev), dv.to(dev), cams.to(dev)
    da = net(imgs, proj, dv)["depth"]
    db = oracle(imgs, proj, dv)["depth"]
    dt = oracle64(imgs.double(), proj.double(), dv.double())["depth"]
    assert rel_l1(da, db) < 1e-3
    assert rel_l1(da.double(), dt) < 1e-3
    la = UnSupLoss()(imgs, cams, da)
    lb = R.unsup_loss(imgs, cams, db)
    assert abs(float(la) - float(lb)) < 1e-3 * abs(float(lb))
    # (a) the loss gradient at ONE depth map (the HIP path's), HIP loss vs oracle loss
    dshared = da.detach().clone().requires_grad_(True)
    dshared_o = da.detach().clone().requires_grad_(True)
    UnSupLoss()(imgs, cams, dshared).backward()
    R.unsup_loss(imgs, cams, dshared_o).backward()
    gdepth = dshared.grad.detach()
    # element by element, robust to the handful of pixels that sit ON a branch point (floor of a sample coordinate, the smooth-L1
    # knee, a top-3 tie): measured on the MI355X (round 3) the two gradients agree to 1e-10 on 6e-5-sized entries except at such
    # pixels, where one entry differs by up to 8 % of the largest gradient
    gdiff = (gdepth - dshared_o.grad).abs()
    gmax = float(dshared_o.grad.abs().max())
    assert float(gdiff.sum() / dshared_o.grad.abs().sum()) < 2e-3
    assert float((gdiff > 1e-9 + 1e-3 * dshared_o.grad.abs()).float().mean()) < 5e-3
    assert float(gdiff.max()) < 0.25 * gmax
    print("config-3 d loss / d depth at the shared depth map: rel-L1 %.2e, max diff %.2e of max %.2e, entries off by > 1e-3: %.2e" % (
        float(gdiff.sum() / dshared_o.grad.abs().sum()), float(gdiff.max()), gmax,
        float((gdiff > 1e-9 + 1e-3 * dshared_o.grad.abs()).float().mean())))
    # (c) first, the fully independent chains (each consumes its own graph): direction and magnitude on every tensor
    ga_full = torch.autograd.grad(la, list(net.parameters()), retain_graph=True)
    gb_full = torch.autograd.grad(lb, list(oracle.parameters()), retain_graph=True)
    names = [k for k, _ in net.named_parameters()]
    worst_cos = (2.0, "")
    for k, ga, gb in zip(names, ga_full, gb_full):
        ga, gb = ga.flatten().double(), gb.flatten().double()
        assert torch.isfinite(ga).all(), k
        if k.endswith("prob.bias") or float(gb.norm()) < 1e-12:
            continue
        cos = float(torch.dot(ga, gb) / (ga.norm() * gb.norm() + 1e-300))
        worst_cos = min(worst_cos, (cos, k))
        if k in ("cost_regularization.conv0.conv.weight", "cost_regularization.prob.weight", "feature.feature.weight"):
            assert cos > 0.98, (k, cos)
            assert 0.8 < float(ga.norm() / (gb.norm() + 1e-300)) < 1.25, k
    print("config-3 independent chains: worst cosine over all parameter tensors %.5f (%s)" % worst_cos)
    # (b) the shared upstream gradient through the three networks: every parameter gradient, fp64-truth criterion
    da.backward(gdepth)
    db.backward(gdepth)
    dt.backward(gdepth.double())
    rep = _check_param_grads(net, oracle, oracle64, ("prob.bias",), "MVSNet N=5 config 3 (shared d loss / d depth)")
    worst = max(rep.items(), key=lambda kv: kv[1][0])
    print("config-3 gradients: worst HIP error %.2e (%s), fp32 torch-ops error there %.2e" % (worst[1][0], worst[0], worst[1][1]))


@pytest.mark.parametrize("cin,cout,ks,stride,hw", [(3, 8, 3, 1, (75, 101)), (8, 8, 3, 1, (64, 96)), (8, 16, 5, 2, (66, 130)),
                                                    (16, 16, 3, 1, (33, 65)), (16, 32, 5, 2, (41, 77)), (32, 32, 3, 1, (32, 40))])
def test_conv2d_family_vs_torch(dev, cin, cout, ks, stride, hw):
    """SURVEY 8(f)-3 first cut (off by default): the feature extractors' 2-D convolution shapes through csrc/conv2d.hip vs
    ATen on the CPU: forward (+ bias), input gradient, weight gradient, ragged sizes, batch 3."""
    from mvs_amd import ops
    g = torch.Generator().manual_seed(cin * 3 + cout + ks)
    x = torch.randn(3, cin, *hw, generator=g)
    w = torch.randn(cout, cin, ks, ks, generator=g) * 0.2
    b = torch.randn(cout, generator=g)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = F.conv2d(xr, wr, br, stride=stride, padding=ks // 2)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy)
    xa, wa, ba = (t.to(dev).requires_grad_(True) for t in (x, w, b))
    y = ops.Conv2dFn.apply(xa, wa, ba, stride)
    y.backward(gy.to(dev))
    assert float((y.cpu() - yr).abs().max()) < 3e-4
    assert float((xa.grad.cpu() - xr.grad).abs().max()) < 5e-4
    assert float((wa.grad.cpu() - wr.grad).abs().max()) < 1e-3 * max(1.0, float(wr.grad.abs().max()))
    assert float((ba.grad.cpu() - br.grad).abs().max()) < 1e-3 * max(1.0, float(br.grad.abs().max()))
    if stride == 2:
        # the input gradient above ran as ONE four-class pass with compacted taps (knob conv2d_s2_mfma = 2, round 6); the four
        # separate parity-class passes (1) and the direct VALU form (0) compute the same sums in other orders
        from mvs_amd import _lib
        lib = _lib.get()
        for form in (1, 0):
            with lib.tuning(conv2d_s2_mfma=form):
                gx = ops.conv2d_dgrad(gy.to(dev), w.to(dev), tuple(x.shape), 2)
            assert float((gx.cpu() - xr.grad).abs().max()) < 5e-4, form


def test_featurenet_hip_convs_vs_stock(dev):
    """FeatureNet with ConvBnReLU.hip_conv (csrc/conv2d.hip) vs the stock MIOpen convolutions: 3 views, 128x160."""
    import copy
    from mvs_amd.jdacs.models import module as MM
    from mvs_amd.jdacs.models.mvsnet import FeatureNet
    torch.manual_seed(2)
    a = FeatureNet().to(dev).train()
    b = copy.deepcopy(a).train()
    x = torch.randn(3, 3, 128, 160, device=dev)
    old = MM.ConvBnReLU.hip_conv
    try:
        MM.ConvBnReLU.hip_conv = False
        yb = b(x, 3)
        yb.square().mean().backward()
        MM.ConvBnReLU.hip_conv = True
        ya = a(x, 3)
        ya.square().mean().backward()
    finally:
        MM.ConvBnReLU.hip_conv = old
    assert float((ya - yb).abs().max()) < 2e-3
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert rel_l1(p.grad, q.grad) < 3e-2, k


def test_featurenet_training_hip_forward_with_fused_statistics(dev):
    """Opt-in training path of the 2-D extractor (ConvBnReLU.hip_fwd_train): forward convolution through csrc/conv2d.hip with
    BatchNorm's partial sums written by its epilogue (mvs_conv2d_fwd_stats + mvs_bn_group_relu_fwd_parts), backward through the
    library -- against the default path (library convolution + BatchNorm kernels with their own statistics pass): outputs,
    parameter gradients and running statistics, 3 views 128x160."""
    import copy
    from mvs_amd import ops
    from mvs_amd.jdacs.models import module as MM
    from mvs_amd.jdacs.models.mvsnet import FeatureNet
    torch.manual_seed(4)
    a = FeatureNet().to(dev).train()
    b = copy.deepcopy(a).train()
    x = torch.randn(3, 3, 128, 160, device=dev).contiguous(memory_format=torch.channels_last)
    c = copy.deepcopy(a).train()
    old_flag, old_async, old_fused, old_split = MM.ConvBnReLU.hip_fwd_train, ops._ASYNC_WGRAD, ops._ASYNC_WGRAD_FUSED, MM.ConvBnReLU.split_bwd
    try:
        ops.set_async_wgrad(False)            # synchronous weight gradients: the comparison is about the kernels
        MM.ConvBnReLU.hip_fwd_train = False
        yb = b(x, 3)
        yb.square().mean().backward()
        torch.cuda.synchronize()
        MM.ConvBnReLU.hip_fwd_train = True
        ya = a(x, 3)
        ya.square().mean().backward()
        torch.cuda.synchronize()
        # regression test of round 3's side-stream mismatch (ops._maybe_on_side_stream): the same path with the library's weight
        # gradients on the side stream, three backward passes in a row, equals the synchronous run
        ops.set_async_wgrad(True)
        MM.ConvBnReLU.split_bwd = True
        for _ in range(3):
            for p_ in c.parameters():
                p_.grad = None
            yc = c(x, 3)
            yc.square().mean().backward()
        torch.cuda.synchronize()
    finally:
        MM.ConvBnReLU.hip_fwd_train, MM.ConvBnReLU.split_bwd = old_flag, old_split
        ops._ASYNC_WGRAD, ops._ASYNC_WGRAD_FUSED = old_async, old_fused
    side_bad = {k: round(rel_l1(p.grad, q.grad), 5) for (k, p), (_, q) in zip(c.named_parameters(), a.named_parameters())
                if not rel_l1(p.grad, q.grad) < 1e-4}
    assert not side_bad, side_bad
    assert float((ya - yb).abs().max()) < 2e-3 * max(1.0, float(yb.abs().max()))
    bad = {k: round(rel_l1(p.grad, q.grad), 4) for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters())
           if not rel_l1(p.grad, q.grad) < 3e-2}
    badbuf = [k for (k, u), (_, v) in zip(a.named_buffers(), b.named_buffers())
              if u.dtype.is_floating_point and not torch.allclose(u, v, rtol=1e-3, atol=1e-4)]
    assert not bad and not badbuf, (bad, badbuf)


def test_conv2d_weight_gradients_one_launch_at_featurenet_size(dev):
    """mvs_conv2d_wgrad_batch at BASELINE config 2's FeatureNet shapes (3 views of 512x640, mvsnet.py:21-32): all eight weight
    gradients from ONE launch + one reduction vs ATen's convolution_backward, parameters channels-last (as bench.py holds them) and
    contiguous; fp32 sums over up to 983 040 positions -> relative L1 1e-4."""
    from mvs_amd import ops
    layers = ((3, 8, 3, 1, 512, 640), (8, 8, 3, 1, 512, 640), (8, 16, 5, 2, 512, 640), (16, 16, 3, 1, 256, 320), (16, 16, 3, 1, 256, 320),
              (16, 32, 5, 2, 256, 320), (32, 32, 3, 1, 128, 160), (32, 32, 3, 1, 128, 160))
    g = torch.Generator().manual_seed(21)
    xs, gys, ws, sts, refs = [], [], [], [], []
    bwd = torch.ops.aten.convolution_backward
    for i, (cin, cout, ks, st, h, w) in enumerate(layers):
        x = torch.randn(3, cin, h, w, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
        wt = (torch.randn(cout, cin, ks, ks, generator=g) * 0.1).to(dev)
        if i % 2 == 0:
            wt = wt.contiguous(memory_format=torch.channels_last)
        ho, wo = (h, w) if st == 1 else ((h - 1) // 2 + 1, (w - 1) // 2 + 1)
        gy = torch.randn(3, cout, ho, wo, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
        refs.append(bwd(gy, x, wt, None, [st, st], [ks // 2, ks // 2], [1, 1], False, [0, 0], 1, [False, True, False])[1])
        xs.append(x); gys.append(gy); ws.append(wt); sts.append(st)
    assert ops.conv2d_wgrad_batch_serves(xs, ws, sts)
    gws = ops.conv2d_wgrad_batch(xs, gys, ws, sts)
    torch.cuda.synchronize()
    for gw, ref, wt, cfg in zip(gws, refs, ws, layers):
        assert gw.stride() == wt.stride(), cfg
        assert rel_l1(gw, ref) < 1e-4, (cfg, rel_l1(gw, ref))


def test_featurenet_training_one_autograd_node_equals_per_block_graph(dev):
    """ops.FeatureExtractorFn (the training extractor as one autograd node, FeatureNet.one_node) launches the same kernels as the
    per-block graph of Conv2dSplitBwdFn / BnReLUFn nodes: outputs, every parameter gradient, running statistics and
    num_batches_tracked agree (statistics are summed with atomics -> not bit-identical), two steps in a row, 3 views 64x96; the
    input gradient too."""
    import copy
    from mvs_amd import ops
    from mvs_amd.jdacs.models.mvsnet import FeatureNet
    torch.manual_seed(14)
    a = FeatureNet().to(dev).train()
    b = copy.deepcopy(a).train()
    xa = torch.randn(3, 3, 64, 96, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    xb = xa.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    old, old_async, old_fused = FeatureNet.one_node, ops._ASYNC_WGRAD, ops._ASYNC_WGRAD_FUSED
    try:
        ops.set_async_wgrad(False)
        for step in range(2):
            FeatureNet.one_node = True
            ya = a(xa, 3)
            assert type(ya.grad_fn).__name__.startswith("FeatureExtractorFn"), type(ya.grad_fn).__name__
            ya.square().mean().backward()
            FeatureNet.one_node = False
            yb = b(xb, 3)
            assert not type(yb.grad_fn).__name__.startswith("FeatureExtractorFn")
            yb.square().mean().backward()
        torch.cuda.synchronize()
    finally:
        FeatureNet.one_node = old
        ops._ASYNC_WGRAD, ops._ASYNC_WGRAD_FUSED = old_async, old_fused
    assert float((ya - yb).abs().max()) < 1e-5 * max(1.0, float(yb.abs().max()))
    assert rel_l1(xa.grad, xb.grad) < 1e-4
    bad = {k: rel_l1(p.grad, q.grad) for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()) if not rel_l1(p.grad, q.grad) < 1e-4}
    badbuf = [k for (k, u), (_, v) in zip(a.named_buffers(), b.named_buffers())
              if not (torch.allclose(u, v, rtol=1e-5, atol=1e-6) if u.dtype.is_floating_point else bool((u == v).all()))]
    assert not bad and not badbuf, (bad, badbuf)


@pytest.mark.parametrize("dgrad_bn", [False, True], ids=["apply_in_consumer", "apply_in_consumer+dgrad_statistics"])
def test_featurenet_training_consumer_side_batchnorm(dev, dgrad_bn):
    """Opt-in ops.FEATURE_FUSED_APPLY (and FEATURE_DGRAD_BNSTATS: the block-below statistics in conv2d.hip's input-gradient epilogue): BatchNorm + ReLU of block i applied inside block i+1's convolution and weight gradient
    (mvs_bn_finalize_slots, mvs_conv2d_fwd_stats_xf, mvs_conv2d_wgrad_batch_xf; no apply pass, no normalised copy for six of the
    seven blocks) against the default one-node path: outputs, input gradient, parameter gradients, running statistics; two steps."""
    import copy
    from mvs_amd import ops
    from mvs_amd.jdacs.models.mvsnet import FeatureNet
    torch.manual_seed(15)
    a = FeatureNet().to(dev).train()
    b = copy.deepcopy(a).train()
    xa = torch.randn(3, 3, 72, 104, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    xb = xa.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    old, old_bn, old_async, old_fused = ops.FEATURE_FUSED_APPLY, ops.FEATURE_DGRAD_BNSTATS, ops._ASYNC_WGRAD, ops._ASYNC_WGRAD_FUSED
    try:
        ops.set_async_wgrad(False)
        for step in range(2):
            ops.FEATURE_FUSED_APPLY, ops.FEATURE_DGRAD_BNSTATS = True, dgrad_bn
            ya = a(xa, 3)
            assert ya.grad_fn.fused
            ya.square().mean().backward()
            ops.FEATURE_FUSED_APPLY, ops.FEATURE_DGRAD_BNSTATS = False, False
            yb = b(xb, 3)
            assert not yb.grad_fn.fused
            yb.square().mean().backward()
        torch.cuda.synchronize()
    finally:
        ops.FEATURE_FUSED_APPLY, ops.FEATURE_DGRAD_BNSTATS = old, old_bn
        ops._ASYNC_WGRAD, ops._ASYNC_WGRAD_FUSED = old_async, old_fused
    assert float((ya - yb).abs().max()) < 1e-5 * max(1.0, float(yb.abs().max()))
    assert rel_l1(xa.grad, xb.grad) < 1e-4
    bad = {k: rel_l1(p.grad, q.grad) for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()) if not rel_l1(p.grad, q.grad) < 1e-4}
    badbuf = [k for (k, u), (_, v) in zip(a.named_buffers(), b.named_buffers())
              if not (torch.allclose(u, v, rtol=1e-5, atol=1e-6) if u.dtype.is_floating_point else bool((u == v).all()))]
    assert not bad and not badbuf, (bad, badbuf)


def test_featurenet_eval_folded_batchnorm_vs_stock(dev):
    """Inference FeatureNet (eval mode, no_grad): BatchNorm folded into the csrc/conv2d.hip convolutions (ConvBnReLU.fold_eval,
    the default) vs the unfolded path (MIOpen convolution + BatchNorm kernel) and vs the oracle's stock modules, 3 views 128x160
    with non-trivial running statistics."""
    import copy
    from mvs_amd.jdacs.models import module as MM
    from mvs_amd.jdacs.models.mvsnet import FeatureNet
    torch.manual_seed(5)
    net = FeatureNet().to(dev)
    x = torch.randn(3, 3, 128, 160, device=dev)
    net.train()
    with torch.no_grad():
        for _ in range(3):
            net(x * (1.0 + 0.1 * torch.randn(1, device=dev)), 3)      # moves the running statistics away from (0, 1)
    net.eval()
    old = MM.ConvBnReLU.fold_eval
    try:
        with torch.no_grad():
            MM.ConvBnReLU.fold_eval = False
            y0 = net(x, 3)
            MM.ConvBnReLU.fold_eval = True
            y1 = net(x, 3)
    finally:
        MM.ConvBnReLU.fold_eval = old
    ref = R.OracleFeatureNet()
    ref.load_state_dict(copy.deepcopy(net.state_dict()))
    ref.eval()
    with torch.no_grad():
        yr = ref(x.cpu())
    scale = float(yr.abs().max())
    assert float((y1 - y0).abs().max()) < 2e-5 * scale
    assert float((y1.cpu() - yr).abs().max()) < 1e-4 * scale


# ---- bf16-storage inference path (BASELINE configs[4]); the reference has no reduced-precision path, so the oracle is the
# fp32 path on the same inputs and the tolerance achieved is stated here -------------------------------
BF16_CONV_CASES = [(32, 8, 1, False, (9, 10, 36)), (8, 8, 1, False, (5, 7, 20)), (16, 16, 1, False, (6, 9, 33)), (32, 32, 1, False, (5, 6, 18)),
                   (64, 64, 1, False, (3, 4, 17)), (8, 1, 1, False, (6, 5, 19)), (8, 16, 2, False, (6, 8, 34)), (16, 32, 2, False, (8, 8, 20)),
                   (32, 64, 2, False, (4, 6, 18)), (64, 32, 2, True, (2, 3, 9)), (32, 16, 2, True, (3, 5, 11)), (16, 8, 2, True, (3, 4, 17))]


@pytest.mark.parametrize("cin,cout,stride,transposed,dims", BF16_CONV_CASES)
def test_conv3d_bf16_inference_vs_torch(dev, cin, cout, stride, transposed, dims):
    """bf16 activations, fp32 accumulation on v_mfma_f32_16x16x32_bf16 vs torch's fp32 convolution of the same bf16-rounded
    operands: the difference is the summation order plus one bf16 rounding of the output (2^-8 relative)."""
    from mvs_amd import ops
    g = torch.Generator().manual_seed(7)
    d, h, w = dims
    x = torch.randn(2, cin, d, h, w, generator=g).bfloat16()
    wshape = (cin, cout, 3, 3, 3) if transposed else (cout, cin, 3, 3, 3)
    wt = torch.randn(wshape, generator=g) * (0.3 / (cin ** 0.5))
    scale = 0.5 + torch.rand(cout, generator=g)
    shift = torch.randn(cout, generator=g) * 0.1
    wr = wt.bfloat16().float()
    if transposed:
        ref = F.conv_transpose3d(x.float(), wr, stride=2, padding=1, output_padding=1)
    else:
        ref = F.conv3d(x.float(), wr, stride=stride, padding=1)
    skip = torch.randn(ref.shape, generator=g).bfloat16()
    exp = torch.relu(ref * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1)) + skip.float()
    xd = x.to(dev).contiguous(memory_format=torch.channels_last_3d)
    with torch.no_grad():
        y = ops.conv3d_forward_bf16(xd, wt.to(dev), stride, transposed, scale=scale.to(dev), shift=shift.to(dev),
                                    skip=skip.to(dev).contiguous(memory_format=torch.channels_last_3d), relu=True)
        yb = ops.conv3d_forward_bf16(xd, wt.to(dev), stride, transposed, shift=shift.to(dev), out_f32=True)
    assert y.dtype == torch.bfloat16 and y.shape == ref.shape
    assert float((y.float().cpu() - exp).abs().max()) <= 2 ** -7 * float(exp.abs().max()) + 1e-5
    assert float((yb.cpu() - (ref + shift.view(1, -1, 1, 1, 1))).abs().max()) < 1e-4 * max(1.0, float(ref.abs().max()))


def test_plane_sweep_variance_bf16_volume(dev):
    """The bf16 volume is the fp32 kernel's value rounded once at the store (same arithmetic): bit-identical to rounding the
    fp32 volume, for every supported view count."""
    from mvs_amd import ops
    g = torch.Generator().manual_seed(3)
    for c, ns, per_pixel, dims in ((32, 2, False, (24, 33, 45)), (16, 6, True, (8, 20, 28)), (32, 3, False, (9, 17, 23)),
                                   (32, 6, False, (16, 30, 44)), (32, 1, False, (7, 12, 20)), (32, 4, True, (8, 16, 24))):
        d, h, w = dims
        rot, trans = _cams(1, ns, h, w)
        ref = torch.randn(1, c, h, w, generator=g).to(dev)
        srcs = [torch.randn(1, c, h, w, generator=g).to(dev) for _ in range(ns)]
        depth = (450 + 30 * torch.rand(1, 1, h, w, generator=g) + 20.0 * torch.arange(d).view(1, d, 1, 1)) if per_pixel \
            else (430 + 9.0 * torch.arange(d)).unsqueeze(0)
        with torch.no_grad():
            v32 = ops.plane_sweep_variance(ref, srcs, rot.to(dev), trans.to(dev), depth.to(dev))
            v16 = ops.plane_sweep_variance(ref, srcs, rot.to(dev), trans.to(dev), depth.to(dev), out_dtype=torch.bfloat16)
        assert v16.dtype == torch.bfloat16 and torch.equal(v16, v32.bfloat16()), (c, ns, per_pixel)


@pytest.mark.parametrize("n,ih,iw,nd", [(3, 256, 320, 96), (7, 1184, 1600, 256)])
def test_bf16_inference_path(dev, n, ih, iw, nd):
    """MVSNet eval with bf16 storage of the cost volume and the regulariser's activations vs the fp32 path on the same inputs
    (and, at the small size, vs the oracle's fp32 torch ops): BASELINE configs[4] at its real size N=7, 1600x1184, D=256.
    Stated tolerance of the bf16 path (measured on the MI355X, random-init model with the x50 logit gain the tests use to make
    the soft-argmin sharp -- a stress case): logits 1e-2 relative L1, depth 1.8e-3 (256x320) / 4.2e-3 (config 5) relative L1
    = 0.4 / 1.2 depth intervals mean absolute; asserted: logits < 3e-2, depth < 1e-2 relative L1 and < 2 intervals.  The fp32
    path itself stays within BASELINE's 1e-3 of the reference."""
    from mvs_amd.jdacs.models.mvsnet import MVSNet
    torch.manual_seed(0)
    net = MVSNet(refine=False)
    with torch.no_grad():
        net.cost_regularization.prob.weight.mul_(50.0)
    imgs, proj, dv = R.synthetic_mvsnet_inputs(1, n, ih, iw, nd, seed=5)
    imgs, proj, dv = imgs.to(dev), proj.to(dev), dv.to(dev)
    net = net.to(dev)
    calibrate_batchnorm(net, imgs, proj, dv)     # running statistics := batch statistics (a non-degenerate eval model)
    cap = {}
    hk = net.cost_regularization.register_forward_hook(lambda m, i, o: cap.update(logits=o.squeeze(1).float()))
    with torch.no_grad():
        o32 = net(imgs, proj, dv)
        l32 = cap["logits"]
        net.storage_dtype = torch.bfloat16
        o16 = net(imgs, proj, dv)
        l16 = cap["logits"]
    hk.remove()
    assert o16["depth"].dtype == torch.float32 and o16["depth"].shape == (1, ih // 4, iw // 4)
    interval = float(dv[0, 1] - dv[0, 0])
    # the comparison only means something on a non-degenerate model: the depth map must actually vary over the image
    assert float(o32["depth"].std()) > 2 * interval and float(l32.std()) > 1e-2
    err = rel_l1(o16["depth"], o32["depth"])
    mad = float((o16["depth"] - o32["depth"]).abs().mean())
    print("bf16 vs fp32 path (N=%d %dx%d D=%d): logits rel-L1 %.2e; depth rel-L1 %.2e, mean abs %.3f mm = %.2f depth intervals "
          "(depth std over the image %.1f mm); confidence mean abs diff %.2e"
          % (n, iw, ih, nd, rel_l1(l16, l32), err, mad, mad / interval, float(o32["depth"].std()),
             float((o16["photometric_confidence"] - o32["photometric_confidence"]).abs().mean())))
    assert rel_l1(l16, l32) < 3e-2            # bf16 storage: 2^-8 per rounding, 11 layers deep
    assert err < 1e-2 and mad < 2.0 * interval
    assert float((o16["photometric_confidence"] - o32["photometric_confidence"]).abs().mean()) < 5e-2
    del o16, o32
    torch.cuda.empty_cache()


def test_config5_batch3_bf16_volume_crosses_2g_elements(dev):
    """BASELINE configs[4] ("in-HBM cost volume exercising 288 GB") at batch 3: the bf16 volume has 3 x 970 M = 2.9 G elements, past
    2^31 -- every kernel of the inference path (sweep store, bf16 regulariser, soft-argmin) must index it with 64-bit arithmetic.
    Eval mode is sample-independent, so each sample of the batch must reproduce its own batch-1 run."""
    from mvs_amd.jdacs.models.mvsnet import MVSNet
    torch.manual_seed(0)
    n, ih, iw, nd = 7, 1184, 1600, 256
    net = MVSNet(refine=False)
    with torch.no_grad():
        net.cost_regularization.prob.weight.mul_(50.0)
    net = net.to(dev)
    ins = [R.synthetic_mvsnet_inputs(1, n, ih, iw, nd, seed=11 + k) for k in range(3)]
    i0, p0, d0 = (t.to(dev) for t in ins[0])
    calibrate_batchnorm(net, i0, p0, d0)
    net.storage_dtype = torch.bfloat16
    singles = []
    with torch.no_grad():
        for im, pr, dv in ins:
            o = net(im.to(dev), pr.to(dev), dv.to(dev))
            singles.append((o["depth"].clone(), o["photometric_confidence"].clone()))
        imgs = torch.cat([t[0] for t in ins]).to(dev)
        proj = torch.cat([t[1] for t in ins]).to(dev)
        dvs = torch.cat([t[2] for t in ins]).to(dev)
        assert 3 * 32 * nd * (ih // 4) * (iw // 4) > 2 ** 31
        ob = net(imgs, proj, dvs)
    torch.cuda.synchronize()
    for k in range(3):
        assert float(singles[k][0].std()) > 1.0                       # a non-degenerate depth map
        assert torch.equal(ob["depth"][k:k + 1], singles[k][0]), "sample %d of the batch differs from its batch-1 run" % k
        assert torch.equal(ob["photometric_confidence"][k:k + 1], singles[k][1])
    del ob, singles, imgs
    torch.cuda.empty_cache()


def test_geo_consistency_filter_golden(dev):
    """the HIP geometric-consistency filter (jdacs/eval.py:169-224 + the aggregation of filter_depth) against the
    fixture produced by EXECUTING the reference's own functions (tests/golden/make_golden_geo.py), and a 1600x1184-sized run
    against the numpy oracle for the masks' statistics."""
    import numpy as np
    from conftest import GOLDEN
    from mvs_amd.jdacs.fusion import geo_filter as GF
    z = np.load(os.path.join(GOLDEN, "g10_geo_filter.npz"))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    nsrc = z["depth_src"].shape[0]
    dref = t(z["depth_ref"])
    srcs = [t(z["depth_src"][v]) for v in range(nsrc)]
    for v in range(nsrc):
        mask, rep, xs, ys = GF.check_geometric_consistency(dref, z["K"][0], z["E"][0], srcs[v], z["K"][v + 1], z["E"][v + 1])
        mask, rep = mask.cpu().numpy(), rep.cpu().numpy()
        assert float((mask != z["mask%d" % (v + 1)]).mean()) < 1e-3            # a pixel exactly at a threshold may flip
        same = mask == z["mask%d" % (v + 1)]
        assert np.allclose(rep[same], z["reproj%d" % (v + 1)][same], rtol=1e-6, atol=1e-4)
        assert np.allclose(xs.cpu().numpy(), z["x_src%d" % (v + 1)], atol=1e-4)
        assert np.allclose(ys.cpu().numpy(), z["y_src%d" % (v + 1)], atol=1e-4)
    r = GF.filter_depth_view(dref, t(z["conf_ref"]), z["K"][0], z["E"][0], srcs, list(z["K"][1:]), list(z["E"][1:]))
    cnt = r["geo_count"].cpu().numpy()
    assert float((cnt != z["geo_count"]).mean()) < 2e-3
    ok = cnt == z["geo_count"]
    assert np.allclose(r["depth_avg"].cpu().numpy()[ok], z["depth_avg"][ok], rtol=1e-6)
    assert float((r["final_mask"].cpu().numpy() != z["final_mask"]).mean()) < 2e-3


def test_filter_depth_scan_level_golden(dev, tmp_path):
    """The scan-level tail of filter_depth (eval.py:340-447) on the GPU vs the fixture made by executing the reference's own function."""
    from conftest import run_filter_depth_golden
    run_filter_depth_golden(tmp_path, "cuda")


def test_fusibile_fusion_kernel_and_folder_run(dev, tmp_path):
    """the fusion kernel of the `fusibile` program (csrc/fusibile.hip; reference jdacs/fusion/fusibile/fusibile.cu:138-277)
    vs oracle/fusibile_np.py at a DTU-like size, per reference camera; then the whole post-processing chain on files -- PFM depth /
    confidence -> probability_filter -> gipuma folder (disp.dmb, fake normals.dmb, "<view>.png.P" cameras) -> depth_map_fusion
    (in process on the GPU instead of the reference's os.system(fusibile)) -> final3d_model.ply -- against the oracle run on the same
    arrays, byte for byte up to the few points whose consistency test sits exactly on a threshold."""
    import numpy as np
    from mvs_amd.jdacs.fusion import depthfusion as DF
    from oracle import fusibile_np as FO
    V, H, W = 5, 120, 160
    Ps, nd, img, Ks, Es = FO.synthetic_scene(V, H, W, seed=4)
    co = FO.fusibile_cameras(Ps)
    lib = __import__("mvs_amd")._lib.get()
    nd_t, img_t = torch.from_numpy(nd).to(dev), torch.from_numpy(img).to(dev)
    cams_t = torch.from_numpy(co["cams"]).to(dev)
    subset = torch.arange(V, dtype=torch.int32, device=dev)
    nthr = float(np.float32(360.0) * np.float32(np.pi) / np.float32(180.0))
    kept = 0
    for ref in range(V):
        out = torch.empty((H, W, 12), dtype=torch.float32, device=dev)
        lib.call("mvs_fusibile_fuse", nd_t.data_ptr(), img_t.data_ptr(), cams_t.data_ptr(), subset.data_ptr(), V, V, H, W, ref,
                 float(co["f"]), 0.25, nthr, 2, 1, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        got = out.cpu().numpy()
        exp, _ = FO.fuse_view(nd, img, co["cams"], list(range(V)), ref, co["f"], 0.25, nthr, 2, True)
        same = (got[..., 0] != 0) == (exp[..., 0] != 0)
        assert same.mean() > 0.999, (ref, same.mean())
        both = same & (exp[..., 0] != 0)
        kept += int(both.sum())
        assert np.abs(got[both] - exp[both]).max() < 1e-3 * np.abs(exp[both]).max()
    assert kept > 0.3 * V * H * W
    # ---- the chain on files ----
    from conftest import build_fusion_folders
    point_folder, ins = build_fusion_folders(tmp_path, V, H, W, seed=4)
    ply = DF.depth_map_fusion(point_folder, "unused-fusibile-exe", 0.25, 2)
    data = open(ply, "rb").read()
    exp_pts = FO.fuse_all(ins["nd"], ins["img"], ins["cams"]["cams"], ins["cams"]["f"], 0.25, nthr, 2)
    head, _, body = data.partition(b"end_header\n")
    n = int(head.split(b"element vertex ")[1].split(b"\n")[0])
    # (a third of the pixels fall to probability_filter: confidence 0.7-1.0 against the 0.8 threshold)
    assert abs(n - exp_pts.shape[0]) <= max(3, exp_pts.shape[0] // 2000) and n > 0.05 * V * H * W and len(body) == 15 * n
    if n == exp_pts.shape[0]:
        rec = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")])
        a, b = np.frombuffer(body, dtype=rec), np.frombuffer(FO.ply_bytes(exp_pts).partition(b"end_header\n")[2], dtype=rec)
        for k in "xyz":
            assert np.allclose(a[k], b[k], rtol=1e-4, atol=1e-2)
        assert float((np.abs(a["r"].astype(int) - b["r"].astype(int)) > 1).mean()) < 1e-3


@pytest.mark.parametrize("cin,cout,hw", [(3, 64, (61, 83)), (64, 64, (37, 65)), (64, 32, (40, 52)), (32, 16, (33, 70)), (16, 16, (45, 37)), (4, 32, (64, 96)),
                                         (32, 1, (64, 96))])
def test_conv2d_lrelu_block_and_wide_channels(dev, cin, cout, hw):
    """the CVP feature pyramid's `conv` block (Conv2d 3x3 + bias + LeakyReLU 0.1, widths up to 64:
    jdacs-ms/models/network.py:16-41) and RefineNet's channel counts (jdacs/models/mvsnet.py:77-92) vs ATen on the same GPU."""
    from mvs_amd import ops
    g = torch.Generator().manual_seed(cin + 7 * cout)
    x = torch.randn(2, cin, *hw, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(cout, cin, 3, 3, generator=g) * (0.5 / cin ** 0.5)).to(dev)
    b = (torch.randn(cout, generator=g) * 0.3).to(dev)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = F.leaky_relu(F.conv2d(xr, wr, br, padding=1), 0.1)
    xa, wa, ba = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = ops.Conv2dLReLUFn.apply(xa, wa, ba, 0.1)
    assert y.shape == yr.shape and float((y - yr).abs().max()) < 3e-4
    gy = torch.randn(yr.shape, generator=g).to(dev)
    yr.backward(gy)
    y.backward(gy)
    assert float((xa.grad - xr.grad).abs().max()) < 5e-4 * max(1.0, float(xr.grad.abs().max()))
    assert float((wa.grad - wr.grad).abs().max()) < 1e-3 * max(1.0, float(wr.grad.abs().max()))
    assert float((ba.grad - br.grad).abs().max()) < 1e-3 * max(1.0, float(br.grad.abs().max()))


def test_feature_pyramid_and_refinenet_hip_convs_vs_stock(dev):
    """FeaturePyramid (jdacs-ms/models/network.py:16-41) with every block through csrc/conv2d.hip, and MVSNet(refine=True)'s
    RefineNet (jdacs/models/mvsnet.py:77-92) with its convolutions through csrc/conv2d.hip == the stock (MIOpen) path."""
    from mvs_amd.jdacs.models.module import ConvBnReLU
    from mvs_amd.jdacs.models.mvsnet import RefineNet
    from mvs_amd.jdacs_ms.models.network import FeaturePyramid
    torch.manual_seed(0)
    fp = FeaturePyramid().to(dev)
    img = torch.randn(1, 3, 96, 160, device=dev)
    old = FeaturePyramid.hip_conv
    try:
        FeaturePyramid.hip_conv = False
        ref = fp(img, 3)
        sum(f.square().mean() for f in ref).backward()
        gref = {k: p.grad.clone() for k, p in fp.named_parameters()}
        fp.zero_grad()
        FeaturePyramid.hip_conv = True
        out = fp(img, 3)
        sum(f.square().mean() for f in out).backward()
    finally:
        FeaturePyramid.hip_conv = old
    for a, b in zip(out, ref):
        assert float((a - b).abs().max()) < 1e-4 * max(1.0, float(b.abs().max()))
    for k, p in fp.named_parameters():
        assert rel_l1(p.grad, gref[k]) < 2e-3, k
    rn = RefineNet().to(dev).train()
    im = torch.randn(2, 3, 128, 192, device=dev)
    d0 = 500 + 100 * torch.rand(2, 32, 48, device=dev)
    oldc = ConvBnReLU.hip_conv
    try:
        ConvBnReLU.hip_conv = False
        r0 = rn(im, d0)
        ConvBnReLU.hip_conv = True
        r1 = rn(im, d0)
    finally:
        ConvBnReLU.hip_conv = oldc
    assert rel_l1(r1, r0) < 1e-5


def test_mvsnet_loss_kernel_vs_reference_formulation(dev):
    """mvsnet_loss on the GPU (one launch forward, one backward) vs F.smooth_l1_loss(est[mask], gt[mask]) as the reference writes it
    (mvsnet.py:164-166), config-2 map size, bool and float masks."""
    from mvs_amd.jdacs.models.mvsnet import mvsnet_loss
    g = torch.Generator().manual_seed(3)
    est0 = 650 + torch.randn(2, 128, 160, generator=g) * 2
    gt = 650 + torch.randn(2, 128, 160, generator=g)
    for mask in ((torch.rand(2, 128, 160, generator=g) > 0.4), (torch.rand(2, 128, 160, generator=g) > 0.4).float()):
        est = est0.clone().to(dev).requires_grad_(True)
        loss = mvsnet_loss(est, gt.to(dev), mask.to(dev))
        loss.backward()
        est_r = est0.clone().requires_grad_(True)
        ref = F.smooth_l1_loss(est_r[mask > 0.5], gt[mask > 0.5], reduction="mean")
        ref.backward()
        assert abs(float(loss) - float(ref)) < 1e-5 * max(1.0, abs(float(ref)))
        assert float((est.grad.cpu() - est_r.grad).abs().max()) < 1e-7
