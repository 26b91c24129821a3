"""CPU: the jdacs-ms self-supervised loss (jdacs-ms/losses/unsup_loss.py:18-82) -- the test-side composition against the
reference's fixtures, the drop-in mvs_amd.jdacs_ms.losses.unsup_loss through the emulated kernels (csrc/unsup_loss.hip,
mvs_unsup_loss_weighted_*), the grid-parallel selection against the single-workgroup one of mvs_unsup_loss_fwd, and the new
entry points' argument checks against the product library."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from emul_util import emul_lib  # noqa: F401
from oracle import ref_torch as R
from unsup_ms_oracle import synthetic_ms_inputs, unsup_loss_ms

torch.set_num_threads(4)
FIXTURES = ["g14_unsup_loss_ms", "g14_unsup_loss_ms_n4"]


@pytest.mark.parametrize("name", FIXTURES)
def test_composition_vs_reference_fixture(name):
    """The test oracle (oracle.ref_torch primitives at full resolution, weights 12 / 6 / 0.05, lambda 1) against the values the
    reference's jdacs-ms UnSupLoss produced (tests/golden/make_golden_unsup_ms.py)."""
    g = load_golden(name)
    depth = g["depth"].clone().requires_grad_(True)
    total, reconstr, ssim, smooth = unsup_loss_ms(g["imgs"], g["cams"], depth, return_terms=True)
    total.backward()
    assert abs(float(total) - float(g["loss"])) < 2e-6 * abs(float(g["loss"]))
    assert abs(float(reconstr) - float(g["reconstr_loss"])) < 2e-6
    assert abs(float(ssim) - float(g["ssim_loss"])) < 2e-6
    assert abs(float(smooth) - float(g["smooth_loss"])) < 2e-5
    gd = g["grad_depth"]
    assert float((depth.grad - gd).abs().max()) < 1e-8 + 1e-4 * float(gd.abs().max())
    kinv, proj = R.unsup_view_transform(g["cams"][:, 0], g["cams"][:, 1])
    warped, mask = R.unsup_inverse_warp(g["imgs"][:, 1].permute(0, 2, 3, 1), kinv, proj, g["depth"])
    assert float((mask - g["mask1"]).abs().mean()) < 1e-3
    both = (mask * g["mask1"]).bool().expand_as(warped)
    assert float((warped - g["warped1"])[both].abs().max()) < 1e-3


@pytest.mark.parametrize("name", FIXTURES)
def test_dropin_golden(emul_lib, name):
    """The drop-in through the emulated kernels vs the reference's fixture: total, the three terms, d loss / d depth with an
    upstream gradient other than 1 (test_emul_kernels.py::test_unsup_loss_golden's tolerances)."""
    from mvs_amd.jdacs_ms.losses.unsup_loss import UnSupLoss
    g = load_golden(name)
    depth = g["depth"].clone().requires_grad_(True)
    crit = UnSupLoss()
    total = crit(g["imgs"], g["cams"], depth)
    (2.0 * total).backward()
    assert crit.unsup_loss is total
    assert abs(float(total) - float(g["loss"])) < 3e-5 * abs(float(g["loss"]))
    assert abs(float(crit.reconstr_loss) - float(g["reconstr_loss"])) < 2e-5
    assert abs(float(crit.ssim_loss) - float(g["ssim_loss"])) < 2e-5
    assert abs(float(crit.smooth_loss) - float(g["smooth_loss"])) < 2e-4
    gd = g["grad_depth"] * 2.0
    assert float((depth.grad - gd).abs().max()) < 4e-6 + 2e-4 * float(gd.abs().max())


def test_dropin_ragged_float64_cams_and_errors(emul_lib):
    """Batch 3, N = 7, 37x53 (B*H*W not a multiple of 256) vs the composition; float64 cameras (what the reference's loader
    yields) give the float32 result; the argument errors."""
    from mvs_amd.jdacs_ms.losses.unsup_loss import UnSupLoss
    imgs, cams, depth = synthetic_ms_inputs(3, 7, 37, 53, seed=6)
    da, db, dc = (depth.clone().requires_grad_(True) for _ in range(3))
    crit = UnSupLoss().to("cpu")
    la = crit(imgs, cams, da)
    terms = (crit.reconstr_loss, crit.ssim_loss, crit.smooth_loss)
    lb, *tb = unsup_loss_ms(imgs, cams, db, return_terms=True)
    la.backward()
    lb.backward()
    assert abs(float(la) - float(lb)) < 3e-5 * abs(float(lb))
    for x, y in zip(terms, tb):
        assert abs(float(x) - float(y)) < 2e-5 * max(1.0, abs(float(y)))
    assert float((da.grad - db.grad).abs().max()) < 4e-6 + 2e-4 * float(db.grad.abs().max())
    assert float(da.grad.abs().max()) > 0
    lc = crit(imgs, cams.double(), dc)
    lc.backward()
    assert torch.equal(lc, la) and torch.equal(dc.grad, da.grad)
    with pytest.raises(ValueError, match="N >= 4"):
        crit(imgs[:, :3], cams[:, :3], depth)
    with pytest.raises(ValueError, match="Different number"):
        crit(imgs, cams[:, :5], depth)
    with pytest.raises(ValueError, match="image resolution"):
        crit(imgs, cams, depth[:, :-1])
    with pytest.raises(ValueError, match="image resolution"):
        crit(imgs, cams, F.interpolate(depth.unsqueeze(1), scale_factor=0.5).squeeze(1))


def _raw_unsup(lib, weighted, ref, views, kinv, proj, depth, lam, weights=(12.0, 6.0, 0.18)):
    """Forward + backward (upstream gradient 1.5) through the C entries on CPU tensors -> out[4], grad, counts, r_v."""
    b, h, w = depth.shape
    nv = len(views)
    arr = (C.c_void_p * nv)(*[v.data_ptr() for v in views])
    pre = "mvs_unsup_loss_weighted" if weighted else "mvs_unsup_loss"
    nws = lib.raw(pre + "_workspace_floats", b, nv, h, w)
    assert nws > 0
    ws = torch.zeros(nws)
    out, g, gd = torch.zeros(4), torch.tensor([1.5]), torch.zeros(b, h, w)
    wts = tuple(weights) if weighted else ()
    lib.call(pre + "_fwd", ref.data_ptr(), arr, kinv.data_ptr(), proj.data_ptr(), depth.data_ptr(), b, nv, h, w, *wts, lam,
             ws.data_ptr(), out.data_ptr(), None)
    lib.call(pre + "_bwd", ref.data_ptr(), arr, kinv.data_ptr(), proj.data_ptr(), depth.data_ptr(), b, nv, h, w, *wts, lam,
             ws.data_ptr(), g.data_ptr(), gd.data_ptr(), None)
    n = b * h * w
    saved = ws[nv * n * 4 + (4 * nv + 2) * ((n + 255) // 256):][:64]
    counts = saved[32:32 + nv].clone()
    icounts = saved[48:48 + nv].clone().view(torch.int32) if weighted else None
    return out, gd, counts, icounts, saved[:nv].clone()


@pytest.mark.parametrize("name", ["g8_unsup_loss", "g8_unsup_loss_n4", "ragged"])
def test_grid_selection_matches_single_workgroup_selection(emul_lib, name):
    """The weighted entry with the jdacs weights (12, 6, 0.18) on quarter-resolution inputs vs mvs_unsup_loss_fwd / _bwd: the
    per-view reconstruction terms and selection counts are identical, the total agrees up to the order of the selected-value
    sum, and the gradient (which reads only the counts) is identical."""
    from mvs_amd import ops
    if name == "ragged":
        imgs, cams, _ = synthetic_ms_inputs(3, 6, 52, 76, seed=9)
        K, _E = R.synthetic_cameras(6, 13, 19, 76)
        cams[:, :, 1, :3, :3] = K
        depth = 600.0 + 60.0 * torch.rand(3, 13, 19, generator=torch.Generator().manual_seed(2))
    else:
        g = load_golden(name)
        imgs, cams, depth = g["imgs"], g["cams"], g["depth"]
    b, n = imgs.shape[:2]
    q = F.interpolate(imgs.reshape(b * n, *imgs.shape[2:]), scale_factor=0.25, mode="bilinear")
    q = q.permute(0, 2, 3, 1).reshape(b, n, q.shape[2], q.shape[3], 3)
    ref, views = q[:, 0].contiguous(), [q[:, v].contiguous() for v in range(1, n)]
    kinv, proj = ops.unsup_view_transforms(cams.float())
    depth = depth.contiguous()
    o_old, g_old, c_old, _, r_old = _raw_unsup(emul_lib, False, ref, views, kinv, proj, depth, 0.7)
    o_new, g_new, c_new, ic_new, r_new = _raw_unsup(emul_lib, True, ref, views, kinv, proj, depth, 0.7)
    assert torch.equal(r_new, r_old)
    assert torch.equal(c_new, c_old) and torch.equal(ic_new.float(), c_old)
    assert int(ic_new.sum()) > 0 and int(ic_new.sum()) <= 3 * depth.numel()
    assert torch.equal(o_new[2:], o_old[2:])
    assert abs(float(o_new[1] - o_old[1])) <= 1e-6 * abs(float(o_old[1]))
    assert abs(float(o_new[0] - o_old[0])) <= 1e-6 * abs(float(o_old[0]))
    assert torch.equal(g_new, g_old)
    # the weights are arguments: other weights move the total and scale the gradient terms
    o_w, g_w, *_ = _raw_unsup(emul_lib, True, ref, views, kinv, proj, depth, 0.7, weights=(24.0, 6.0, 0.18))
    assert abs(float(o_w[0]) - float(24.0 * o_new[1] + 6.0 * o_new[2] + 0.18 * o_new[3])) < 1e-5 * abs(float(o_w[0]))
    assert not torch.equal(g_w, g_new)


def test_weighted_entry_argument_errors_and_workspace():
    """mvs_unsup_loss_weighted_*: null pointers, V = 2 / 11, H < 3, too many pixels are rejected before any launch with a
    message naming the limit; the workspace query's values (product library, no GPU needed)."""
    from mvs_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.MvsLib()
    dummy = C.c_void_p(64)          # never dereferenced: validation happens before any launch
    views = (C.c_void_p * 11)(*([64] * 11))
    ptrs = (dummy, views, dummy, dummy, dummy)
    w = (12.0, 6.0, 0.05, 1.0)
    cases = [
        ((None, views, dummy, dummy, dummy, 1, 4, 8, 8), "null"),
        ((dummy, None, dummy, dummy, dummy, 1, 4, 8, 8), "null"),
        ((dummy, views, dummy, dummy, None, 1, 4, 8, 8), "null"),
        (ptrs + (1, 2, 8, 8), "3 <= V <= 10"),
        (ptrs + (1, 11, 8, 8), "3 <= V <= 10"),
        (ptrs + (1, 4, 2, 8), "H >= 3 and W >= 3"),
        (ptrs + (1, 4, 8, 2), "H >= 3 and W >= 3"),
        (ptrs + (0, 4, 8, 8), "B >= 1"),
        (ptrs + (33, 4, 4096, 4000), "UNSUP_MAX_PIXELS"),
    ]
    for args, msg in cases:
        with pytest.raises(ValueError, match=msg):
            lib.call("mvs_unsup_loss_weighted_fwd", *args, *w, dummy, dummy, None)
        with pytest.raises(ValueError, match=msg):
            lib.call("mvs_unsup_loss_weighted_bwd", *args, *w, dummy, dummy, dummy, None)
    with pytest.raises(ValueError, match="null output"):
        lib.call("mvs_unsup_loss_weighted_fwd", *ptrs, 1, 4, 8, 8, *w, dummy, None, None)
    with pytest.raises(ValueError, match="null gradient"):
        lib.call("mvs_unsup_loss_weighted_bwd", *ptrs, 1, 4, 8, 8, *w, dummy, None, dummy, None)
    q = lambda *s: lib.raw("mvs_unsup_loss_weighted_workspace_floats", *s)
    for bad in ((1, 2, 8, 8), (1, 11, 8, 8), (1, 4, 2, 8), (1, 4, 8, 2), (0, 4, 8, 8), (33, 4, 4096, 4000)):
        assert q(*bad) == -1, bad
    for b, v, h, w_ in ((2, 4, 16, 20), (1, 3, 45, 61), (4, 6, 128, 160), (1, 10, 3, 3)):
        n = b * h * w_
        nblk = (n + 255) // 256
        assert q(b, v, h, w_) == lib.raw("mvs_unsup_loss_workspace_floats", b, v, h, w_) + 64 + (v + 1) * nblk
        assert q(b, v, h, w_) == v * n * 4 + (4 * v + 2) * nblk + 64 + 2 * b * (h - 2) * (w_ - 2) * 9 + 64 + (v + 1) * nblk
    assert q(32, 10, 4096, 4096) > 0 and q(32, 10, 4096, 4097) == -1     # 2^29 pixels is the largest admitted


@pytest.mark.skipif(os.environ.get("MVS_EMUL_FULL") != "1", reason="10 minutes of emulation; set MVS_EMUL_FULL=1 (the GPU version is test_gpu_unsup_loss_ms.py::test_jdacs_ms_self_supervised_step_recipe_shape)")
def test_cvp_self_supervised_step_end_to_end(emul_lib):
    """A jdacs-ms self-supervised step in miniature (N = 4, nscale 2, 32x40): CVPMVSNet forward -> each level's depth map
    nearest-up-sampled to the image size (train.py:227) -> UnSupLoss -> sum -> backward into the network, every kernel of the
    path in one graph, vs OracleCVPMVSNet + the composition."""
    from mvs_amd.jdacs_ms.losses.unsup_loss import UnSupLoss
    from mvs_amd.jdacs_ms.models.network import CVPMVSNet
    torch.manual_seed(0)
    b, n, h, w = 1, 4, 32, 40
    args = R.cvp_args(nsrc=n - 1, nscale=2, mode="train")
    net = CVPMVSNet(args)
    oracle = R.OracleCVPMVSNet(args)
    oracle.load_state_dict(net.state_dict())
    net.train()
    oracle.train()
    imgs, cams, _ = synthetic_ms_inputs(b, n, h, w, seed=7)
    K, E = cams[:, :, 1, :3, :3], cams[:, :, 0]
    ins = [t.contiguous() for t in (imgs[:, 0], imgs[:, 1:], K[:, 0], K[:, 1:], E[:, 0], E[:, 1:])] + \
          [torch.tensor([600.0] * b), torch.tensor([680.0] * b)]
    crit = UnSupLoss()
    oa = net(*ins)["depth_est_list"]
    ob = oracle(*ins)["depth_est_list"]
    la = sum(crit(imgs, cams, F.interpolate(d.unsqueeze(1), size=[h, w]).squeeze(1)) for d in oa)
    lb = sum(unsup_loss_ms(imgs, cams, F.interpolate(d.unsqueeze(1), size=[h, w]).squeeze(1)) for d in ob)
    la.backward()
    lb.backward()
    assert abs(float(la) - float(lb)) < 1e-4 * abs(float(lb))
    pa, pb = dict(net.named_parameters()), dict(oracle.named_parameters())
    checked = 0
    for k in pb:
        if k.endswith("prob0.bias") or pb[k].grad is None or float(pb[k].grad.abs().max()) == 0:
            continue
        cos = float(torch.nn.functional.cosine_similarity(pa[k].grad.flatten().double(), pb[k].grad.flatten().double(), 0))
        assert cos > 0.98, (k, cos)
        checked += 1
    assert checked >= 10
