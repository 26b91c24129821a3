"""GPU (MI355X): the JDACS co-segmentation loss (csrc/seg_loss_kernels.h: mvs_nmf_solve, mvs_seg_loss_*) against the reference's
fixtures, against the test oracle at the training shape (N = 7, features [7,512,14,14], depth 128x160, B = 1 and 4), its
determinism, and that solve + loss forward + backward are enqueued without a host synchronisation."""
import pytest
import torch

from conftest import assert_as_accurate_as_fp32_reference, load_golden
import seg_oracle as S
from test_seg_loss import NMF_CASES, SEG_FIXTURES, nmf_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    from mvs_amd import _lib
    _lib._INSTANCE = None
    lib = _lib.get()
    assert lib.raw("mvs_is_emulation") == 0  # the product library, not the test emulation
    return torch.device("cuda:0")


@pytest.mark.parametrize("fixture,prefix", NMF_CASES)
def test_nmf_solve_vs_fixture(dev, fixture, prefix):
    """tests/test_seg_loss.py::test_nmf_solve_emulated_vs_fixture on the device."""
    from mvs_amd import ops
    c = nmf_case(fixture, prefix)
    V, upd = c["V"], bool(c["update_h"])
    W64, H64, it64, _, e0_64, el_64 = S.nmf_iterate(V.double(), c["W0"], c["H0"], upd, c["max_iter"], c["tol"])
    W, H, status = ops.nmf_solve(V.to(dev), c["W0"].to(dev), c["H0"].to(dev), update_h=upd, max_iter=c["max_iter"], tol=c["tol"])
    W, H, status = W.cpu(), H.cpu(), status.cpu()
    assert int(status[0, 0]) == c["iters"] == it64 and float(status[0, 1]) == 0.0
    assert abs(float(status[0, 2]) - e0_64) <= 1e-5 * e0_64 and abs(float(status[0, 3]) - el_64) <= 1e-5 * el_64
    print("%s W err ours %.3e reference %.3e; H ours %.3e reference %.3e" % (
        prefix, float((W - W64).abs().max()), float((c["W"] - W64).abs().max()), float((H - H64).abs().max()),
        float((c["H"] - H64).abs().max())))
    assert_as_accurate_as_fp32_reference(W, c["W"], W64, what=prefix + "W")
    if upd:
        assert_as_accurate_as_fp32_reference(H, c["H"], H64, what=prefix + "H")
    else:
        assert torch.equal(H, c["H0"])
    zr, zc = V.sum(1) == 0, V.sum(0) == 0
    assert bool((W[zr] == 0).all()) and bool((H[:, zc] == 0).all())


@pytest.mark.parametrize("name", SEG_FIXTURES)
def test_seg_loss_vs_fixture(dev, name):
    """tests/test_seg_loss.py::test_seg_loss_emulated_vs_fixture on the device."""
    from mvs_amd import ops
    g = load_golden(name)
    kinv, proj = ops.unsup_view_transforms(g["cams"].to(dev))
    nv = g["view_segs"].shape[1]
    depth = g["depth"].to(dev).requires_grad_(True)
    views = [g["view_segs"][:, v].to(dev) for v in range(nv)]
    total, per_view = ops.seg_loss(depth, g["ref_seg"].to(dev), views, kinv, proj)
    (2.0 * total).backward()
    total, per_view = total.detach().cpu(), per_view.cpu()
    assert abs(float(total) - float(g["loss"])) < 3e-5 * abs(float(g["loss"]))
    assert bool(((per_view - g["per_view"]).abs() < 3e-5 * g["per_view"].abs()).all())
    gd = 2.0 * g["grad_depth"]
    print(name, "grad err %.3e of max %.3e" % (float((depth.grad.cpu() - gd).abs().max()), float(gd.abs().max())))
    assert float((depth.grad.cpu() - gd).abs().max()) <= 2e-4 * float(gd.abs().max())


def test_segdff_and_unsupsegloss_end_to_end(dev):
    """images -> stand-in network -> SegDFF -> UnSupSegLoss on the device.  SegDFF draws its initial factors from a generator of
    the tensor's device, so the fixture's CPU-seeded heat maps are not what a device run produces (the reference on a GPU differs
    from its CPU run in the same way); the fixture provides the inputs, and the yardstick is seg_oracle on the CPU started from the
    SAME device-drawn factors: heat maps by the project's criterion (fp64 truth, fp32 reference), loss and gradient on those maps
    by the fixture tolerances."""
    import torch.nn.functional as F
    from mvs_amd.jdacs.losses.unsup_seg_loss import UnSupSegLoss
    from mvs_amd.jdacs.models.seg_dff import initial_factors
    g = load_golden("g15_seg_e2e")
    k = int(g["K"])
    net = S.StandInNet(seed=int(g["net_seed"])).to(dev)
    crit = UnSupSegLoss(k, net=net)
    imgs = g["imgs"].to(dev)
    b, nv = imgs.shape[:2]
    heat = crit.seg_model(imgs)
    assert tuple(heat.shape) == tuple(g["heatmaps"].shape) and not heat.requires_grad
    with torch.no_grad():
        f = net.features(F.interpolate(imgs.reshape(b * nv, *imgs.shape[2:]), size=(224, 224), mode="bilinear", align_corners=False))
        flat = f.permute(0, 2, 3, 1).reshape(b, -1, f.shape[1])
    for i in range(b):
        W0, H0 = initial_factors(flat[i], k, 1)
        r32 = S.nmf_iterate(flat[i].cpu(), W0.cpu(), H0.cpu(), True, 50, 1e-4)
        r64 = S.nmf_iterate(flat[i].cpu().double(), W0.cpu(), H0.cpu(), True, 50, 1e-4)
        assert S.stopping_tests_clear_of_tol(r32[3], 1e-4) and S.stopping_tests_clear_of_tol(r64[3], 1e-4) and r32[2] == r64[2]
        assert_as_accurate_as_fp32_reference(heat[i].cpu().reshape(-1, k), r32[0], r64[0], what="heat[%d]" % i)
    assert S.seg_inputs_well_conditioned(heat.cpu(), g["cams"], g["depth"])
    d_ref = g["depth"].clone().requires_grad_(True)
    t_ref = S.seg_loss(heat.cpu(), g["cams"], d_ref)
    (2.0 * t_ref).backward()
    depth = g["depth"].to(dev).requires_grad_(True)
    total, ref_seg, view_segs = crit(imgs, g["cams"].to(dev), depth)
    (2.0 * total).backward()
    assert tuple(ref_seg.shape) == tuple(g["ref_seg"].shape) and tuple(view_segs.shape) == tuple(g["view_segs"].shape)
    assert abs(float(total.detach()) - float(t_ref.detach())) < 3e-5 * abs(float(t_ref.detach()))
    assert float((depth.grad.cpu() - d_ref.grad).abs().max()) <= 2e-4 * float(d_ref.grad.abs().max())


def training_inputs(b, seed):
    """V [B,1372,512] under the stopping-test condition, cameras and a 128x160 depth map (the maps come from the solve)."""
    Vs, facs = [], []
    s = seed
    while len(Vs) < b:
        V = S.relu_like_matrix(7 * 14 * 14, 512, 4, s)
        W0, H0 = S.nmf_initial_factors(V, 4, 1)
        r32 = S.nmf_iterate(V, W0, H0, True, 50, 1e-4)
        r64 = S.nmf_iterate(V.double(), W0, H0, True, 50, 1e-4)
        if S.stopping_tests_clear_of_tol(r32[3], 1e-4) and S.stopping_tests_clear_of_tol(r64[3], 1e-4) and r32[2] == r64[2]:
            Vs.append(V)
            facs.append((W0, H0, r32, r64))
        s += 1
    return torch.stack(Vs), facs


@pytest.mark.parametrize("b", [1, 4])
def test_training_shape_vs_oracle(dev, b):
    """B = 1 and 4, N = 7, features [7,512,14,14] -> V [B,1372,512], depth 128x160, inputs built on the fly under the three
    input conditions: the solve against seg_oracle's fp64 (truth) and fp32 (reference) iteration on the CPU by the project's
    criterion; the loss and its gradient on the solve's maps against seg_oracle's fp32 composition by the fixture tolerances."""
    from mvs_amd import ops
    V, facs = training_inputs(b, seed=50 + b)
    W0 = torch.stack([f[0] for f in facs])
    H0 = torch.stack([f[1] for f in facs])
    W, H, status = ops.nmf_solve(V.to(dev), W0.to(dev), H0.to(dev), max_iter=50, tol=1e-4)
    Wc, Hc, status = W.cpu(), H.cpu(), status.cpu()
    for i, (_, _, r32, r64) in enumerate(facs):
        assert int(status[i, 0]) == r32[2] == r64[2] and float(status[i, 1]) == 0.0
        assert_as_accurate_as_fp32_reference(Wc[i], r32[0], r64[0], what="W[%d]" % i)
        assert_as_accurate_as_fp32_reference(Hc[i], r32[1], r64[1], what="H[%d]" % i)
    heat, cams, depth = S.conditioned_seg_inputs(Wc.view(b, 7, 14, 14, 4), b, 7, 128, 160, seed=70 + b)
    # the three input conditions, the coordinate one for every integer (seg_oracle.conditioned_seg_inputs says why)
    assert S.seg_inputs_well_conditioned(heat, cams, depth) and S.coordinates_clear_of_integers(cams, depth)
    d_ref = depth.clone().requires_grad_(True)
    t_ref, terms_ref = S.seg_loss(heat, cams, d_ref, return_parts=True)[:2]
    (2.0 * t_ref).backward()
    ref_seg, view_segs = S.maps_at_depth_resolution(heat.to(dev), 128, 160)
    kinv, proj = ops.unsup_view_transforms(cams.to(dev))
    d = depth.to(dev).requires_grad_(True)
    total, per_view = ops.seg_loss(d, ref_seg, [view_segs[:, v] for v in range(6)], kinv, proj)
    (2.0 * total).backward()
    t_ref, terms_ref = t_ref.detach(), terms_ref.detach()
    print("B=%d loss %.7f vs %.7f; grad err %.3e of max %.3e" % (b, float(total.detach()), float(t_ref),
                                                               float((d.grad.cpu() - d_ref.grad).abs().max()), float(d_ref.grad.abs().max())))
    assert abs(float(total.detach()) - float(t_ref)) < 3e-5 * abs(float(t_ref))
    assert bool(((per_view.cpu() - terms_ref).abs() < 3e-5 * terms_ref.abs()).all())
    assert float((d.grad.cpu() - d_ref.grad).abs().max()) <= 2e-4 * float(d_ref.grad.abs().max())


def _device_case(dev, b=2):
    g = torch.Generator().manual_seed(5)
    V = torch.stack([S.relu_like_matrix(1372, 512, 4, 90 + i) for i in range(b)])
    facs = [S.nmf_initial_factors(V[i], 4, 1) for i in range(b)]
    W0, H0 = torch.stack([f[0] for f in facs]), torch.stack([f[1] for f in facs])
    seg, cams, depth = S.conditioned_seg_inputs(torch.rand(b, 7, 14, 14, 4, generator=g) * 2, b, 7, 128, 160, seed=91)
    return V.to(dev), W0.to(dev), H0.to(dev), seg.to(dev), cams.to(dev), depth.to(dev)


def test_two_runs_identical_bits_and_no_host_sync(dev):
    """The solve, the loss forward and its backward() run under torch.cuda.set_sync_debug_mode("error") (any host
    synchronisation raises); a second run gives the same bits."""
    from mvs_amd import ops
    V, W0, H0, seg, cams, depth = _device_case(dev)
    ref_seg, view_segs = S.maps_at_depth_resolution(seg, 128, 160)
    views = [view_segs[:, v].contiguous() for v in range(6)]
    ref_seg = ref_seg.contiguous()
    kinv, proj = ops.unsup_view_transforms(cams)
    scale = torch.full((), 2.0, device=dev)
    outs = []
    ops.nmf_solve(V, W0, H0)                       # first use: library load, allocator warm-up
    torch.cuda.synchronize()
    for _ in range(2):
        d = depth.clone().requires_grad_(True)
        torch.cuda.set_sync_debug_mode("error")
        try:
            W, H, status = ops.nmf_solve(V, W0, H0, max_iter=50, tol=1e-4)
            total, per_view = ops.seg_loss(d, ref_seg, views, kinv, proj)
            (total * scale).backward()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        outs.append([t.detach().cpu() for t in (W, H, status, total, per_view, d.grad)])
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    assert bool(torch.isfinite(outs[0][3])) and float(outs[0][5].abs().max()) > 0 and int(outs[0][2][0, 0]) == 50
