"""CPU: the JDACS co-segmentation loss -- the test-side restatement (tests/seg_oracle.py) against the reference's fixtures
(tests/golden/g15_*.npz), ops.nmf_solve / ops.seg_loss and the drop-ins (SegDFF, UnSupSegLoss, aug_loss, random_image_mask)
through the emulated kernels (csrc/seg_loss_kernels.h), and the new entry points' argument checks against the product library."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import assert_as_accurate_as_fp32_reference, load_golden
from emul_util import emul_lib  # noqa: F401
import seg_oracle as S

torch.set_num_threads(4)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NMF_CASES = [("g15_nmf_small", "ragged_"), ("g15_nmf_small", "k3_"), ("g15_nmf_small", "early_"), ("g15_nmf_small", "fixedh_"),
             ("g15_nmf_train", "train_")]
SEG_FIXTURES = ["g15_seg_loss", "g15_seg_loss_odd"]


def nmf_case(fixture, prefix):
    g = load_golden(fixture)
    c = {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}
    c["V"] = c["Vq"].float() / 32.0
    for k in ("iters", "max_iter", "update_h"):
        c[k] = int(c[k])
    c["tol"] = float(c["tol"])
    return c


@pytest.mark.parametrize("fixture,prefix", NMF_CASES)
def test_oracle_nmf_vs_reference_fixture(fixture, prefix):
    """seg_oracle's fp32 iteration against what the reference's NMF returned: same iteration count, W and H within
    4e-6 * max|W| (four times the fp32-vs-fp64 difference; bit equality on the generating CPU is asserted by the generator)."""
    c = nmf_case(fixture, prefix)
    W, H, iters, tests, e0, elast = S.nmf_iterate(c["V"], c["W0"], c["H0"], bool(c["update_h"]), c["max_iter"], c["tol"])
    assert iters == c["iters"]
    bound = 4e-6 * float(c["W"].abs().max())
    assert float((W - c["W"]).abs().max()) <= bound and float((H - c["H"]).abs().max()) <= bound
    assert S.stopping_tests_clear_of_tol(tests, c["tol"])
    assert abs(e0 - float(c["e0"])) <= 1e-5 * e0 and abs(elast - float(c["e_last"])) <= 1e-5 * elast


@pytest.mark.parametrize("name", SEG_FIXTURES)
def test_oracle_seg_loss_vs_reference_fixture(name):
    """The composition from the oracle's warp primitives against the reference's UnSupSegLoss.forward
    (tests/test_unsup_loss_ms.py::test_composition_vs_reference_fixture's tolerances, the gradient bound relative only)."""
    g = load_golden(name)
    assert S.seg_inputs_well_conditioned(g["seg"], g["cams"], g["depth"])
    depth = g["depth"].clone().requires_grad_(True)
    total, terms, ref_seg, view_segs, warped1, mask1 = S.seg_loss(g["seg"], g["cams"], depth, return_parts=True)
    total.backward()
    total = total.detach()
    assert abs(float(total) - float(g["loss"])) < 2e-6 * abs(float(g["loss"]))
    assert float((terms.detach() - g["per_view"]).abs().max()) < 2e-6
    assert float((ref_seg - g["ref_seg"]).abs().max()) < 2e-6 and float((view_segs - g["view_segs"]).abs().max()) < 2e-6
    gd = g["grad_depth"]
    assert float((depth.grad - gd).abs().max()) < 1e-4 * float(gd.abs().max())
    assert float((mask1 - g["mask1"]).abs().mean()) < 1e-3
    both = (mask1 * g["mask1"]).bool().expand_as(warped1)
    assert float((warped1.detach() - g["warped1"])[both].abs().max()) < 1e-3


@pytest.mark.parametrize("fixture,prefix", NMF_CASES)
def test_nmf_solve_emulated_vs_fixture(emul_lib, fixture, prefix):
    """ops.nmf_solve through the emulated kernels: the reference's iteration count; W and H as accurate against the fp64
    iteration as the reference's own fp32 result (the project's criterion, default slack); all-zero rows / columns of V stay
    exactly zero in W / H; the status row."""
    from mvs_amd import ops
    c = nmf_case(fixture, prefix)
    V, upd = c["V"], bool(c["update_h"])
    W64, H64, it64, _, e0_64, el_64 = S.nmf_iterate(V.double(), c["W0"], c["H0"], upd, c["max_iter"], c["tol"])
    W0, H0 = c["W0"].clone(), c["H0"].clone()
    W, H, status = ops.nmf_solve(V, W0, H0, update_h=upd, max_iter=c["max_iter"], tol=c["tol"])
    assert torch.equal(W0, c["W0"]) and torch.equal(H0, c["H0"])            # the initial factors are not modified
    assert tuple(status.shape) == (1, 4)
    assert int(status[0, 0]) == c["iters"] == it64
    assert float(status[0, 1]) == 0.0
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
    if prefix == "ragged_":
        assert int(zr.sum()) >= 5 and int(zc.sum()) >= 5
    assert bool((W[zr] == 0).all()) and bool((H[:, zc] == 0).all())
    assert bool((W >= 0).all()) and bool((H >= 0).all())


def test_nmf_solve_batch_tol_off_and_deterministic(emul_lib):
    """Two problems in one call equal the two single calls bit for bit (also when only one of them stops early); tol <= 0 runs
    max_iter iterations and reports e0 as the last error; k = 1 and k = 8; a second run gives identical bits."""
    from mvs_amd import ops
    a, b = nmf_case("g15_nmf_small", "early_"), nmf_case("g15_nmf_small", "k3_")
    n, m = 150, 50
    Va, Vb = a["V"][:n, :m].contiguous(), b["V"][:n, :m].contiguous()
    Wa, Ha = S.nmf_initial_factors(Va, 4, 1)
    Wb, Hb = S.nmf_initial_factors(Vb, 4, 2)
    W, H, st = ops.nmf_solve(torch.stack([Va, Vb]), torch.stack([Wa, Wb]), torch.stack([Ha, Hb]), max_iter=23, tol=5e-2)
    for i, (V1, W1, H1) in enumerate(((Va, Wa, Ha), (Vb, Wb, Hb))):
        Ws, Hs, ss = ops.nmf_solve(V1, W1, H1, max_iter=23, tol=5e-2)
        assert torch.equal(W[i], Ws) and torch.equal(H[i], Hs) and torch.equal(st[i], ss[0])
        _, _, iters, _, _, _ = S.nmf_iterate(V1, W1, H1, True, 23, 5e-2)
        assert int(st[i, 0]) == iters
    W2, H2, st2 = ops.nmf_solve(torch.stack([Va, Vb]), torch.stack([Wa, Wb]), torch.stack([Ha, Hb]), max_iter=23, tol=5e-2)
    assert torch.equal(W, W2) and torch.equal(H, H2) and torch.equal(st, st2)
    Wn, Hn, sn = ops.nmf_solve(Va, Wa, Ha, max_iter=12, tol=0.0)
    Wo, Ho, _, _, e0, _ = S.nmf_iterate(Va.double(), Wa, Ha, True, 12, 0.0)
    assert int(sn[0, 0]) == 12 and float(sn[0, 2]) == float(sn[0, 3]) and abs(float(sn[0, 2]) - e0) < 1e-5 * e0
    assert float((Wn - Wo).abs().max()) < 1e-5 * float(Wo.abs().max())
    for k in (1, 8):
        Wk, Hk = S.nmf_initial_factors(Va, k, 3)
        Wr, Hr, sr = ops.nmf_solve(Va, Wk, Hk, max_iter=11, tol=1e-4)
        Wo, Ho, iters, _, _, _ = S.nmf_iterate(Va.double(), Wk, Hk, True, 11, 1e-4)
        assert int(sr[0, 0]) == iters
        assert float((Wr - Wo).abs().max()) < 2e-5 * float(Wo.abs().max()) and float((Hr - Ho).abs().max()) < 2e-5 * float(Ho.abs().max())


def test_nmf_solve_counts_non_finite_entries(emul_lib):
    """An infinite entry of V makes its row of W non-finite: status[1] counts it (what SegDFF's retry reads)."""
    from mvs_amd import ops
    c = nmf_case("g15_nmf_small", "k3_")
    V = c["V"][:64, :32].clone()
    V[5, 7] = float("inf")
    W0, H0 = S.nmf_initial_factors(c["V"][:64, :32], 3, 1)
    W, _, st = ops.nmf_solve(V, W0, H0, max_iter=3, tol=1e-4)
    assert float(st[0, 1]) == float((~torch.isfinite(W)).sum()) > 0


@pytest.mark.parametrize("name", SEG_FIXTURES)
def test_seg_loss_emulated_vs_fixture(emul_lib, name):
    """ops.seg_loss on the reference's own up-sampled maps: total and per-view terms to a relative 3e-5, the depth gradient
    (upstream gradient 2) by max|diff| <= 2e-4 * max|g_ref| -- no absolute floor: the gradients here are of order 1e-6."""
    from mvs_amd import ops
    g = load_golden(name)
    kinv, proj = ops.unsup_view_transforms(g["cams"])
    nv = g["view_segs"].shape[1]
    depth = g["depth"].clone().requires_grad_(True)
    total, per_view = ops.seg_loss(depth, g["ref_seg"], [g["view_segs"][:, v] for v in range(nv)], kinv, proj)
    (2.0 * total).backward()
    total = total.detach()
    print(name, float(total), float(g["loss"]), per_view.tolist(), g["per_view"].tolist())
    assert abs(float(total) - float(g["loss"])) < 3e-5 * abs(float(g["loss"]))
    assert bool(((per_view - g["per_view"]).abs() < 3e-5 * g["per_view"].abs()).all())
    assert not per_view.requires_grad
    gd = 2.0 * g["grad_depth"]
    print(name, "grad err %.3e of max %.3e" % (float((depth.grad - gd).abs().max()), float(gd.abs().max())))
    assert float((depth.grad - gd).abs().max()) <= 2e-4 * float(gd.abs().max())
    # a view nobody sees: 0 / 0 = nan for its term and the total, like F.cross_entropy on an empty selection
    far = proj.clone()
    far[:, 0, 3] += 1e9
    t2, pv2 = ops.seg_loss(g["depth"], g["ref_seg"], [g["view_segs"][:, v] for v in range(nv)], kinv, far)
    assert bool(torch.isnan(pv2[0])) and bool(torch.isnan(t2)) and bool(torch.isfinite(pv2[1:]).all())


def test_segdff_and_unsupsegloss_end_to_end(emul_lib):
    """images -> stand-in network -> SegDFF (one batched NMF solve, seed 1) -> UnSupSegLoss, against the reference's NMF +
    UnSupSegLoss.forward on the same features.  Heat maps within 1e-4 * max (the features come from a stock convolution whose
    summation order may differ between CPUs by ~1e-7; fifty multiplicative updates carry that to ~1e-6, as the measured
    fp32-vs-fp64 difference shows; two orders above it), loss to 3e-5, gradient to 2e-4 of its maximum."""
    from mvs_amd.jdacs.losses.unsup_seg_loss import UnSupSegLoss
    from mvs_amd.jdacs.models.seg_dff import SegDFF
    from mvs_amd.jdacs_ms.losses.unsup_seg_loss import UnSupSegLoss as UnSupSegLossMs
    from mvs_amd.jdacs_ms.models.seg_dff import SegDFF as SegDFFMs
    assert UnSupSegLossMs is UnSupSegLoss and SegDFFMs is SegDFF
    g = load_golden("g15_seg_e2e")
    k = int(g["K"])
    net = S.StandInNet(seed=int(g["net_seed"]))
    seed_before = torch.initial_seed()
    state_before = torch.get_rng_state()
    heat = SegDFF(k, max_iter=50, net=net)(g["imgs"])
    assert torch.initial_seed() == seed_before and torch.equal(torch.get_rng_state(), state_before)   # private generator
    assert tuple(heat.shape) == tuple(g["heatmaps"].shape) and not heat.requires_grad
    assert float((heat - g["heatmaps"]).abs().max()) <= 1e-4 * float(g["heatmaps"].abs().max())
    crit = UnSupSegLoss(k, net=net)
    depth = g["depth"].clone().requires_grad_(True)
    total, ref_seg, view_segs = crit(g["imgs"], g["cams"], depth)
    (2.0 * total).backward()
    total = total.detach()
    assert tuple(ref_seg.shape) == tuple(g["ref_seg"].shape) and tuple(view_segs.shape) == tuple(g["view_segs"].shape)
    assert float((ref_seg - g["ref_seg"]).abs().max()) <= 1e-4 * float(g["ref_seg"].abs().max())
    assert abs(float(total) - float(g["loss"])) < 3e-5 * abs(float(g["loss"]))
    gd = 2.0 * g["grad_depth"]
    print("e2e loss %.7f vs %.7f; grad err %.3e of max %.3e" % (float(total), float(g["loss"]),
                                                             float((depth.grad - gd).abs().max()), float(gd.abs().max())))
    assert float((depth.grad - gd).abs().max()) <= 2e-4 * float(gd.abs().max())

    class Args:
        seg_clusters = k
    assert UnSupSegLoss(Args(), net=net).seg_model.K == k
    with pytest.raises(ValueError, match="Different number"):
        crit(g["imgs"], g["cams"][:, :2], depth)


def test_compute_seg_loss_plain_torch():
    from mvs_amd.jdacs.losses.unsup_seg_loss import compute_seg_loss
    g = load_golden("g15_seg_loss")
    assert abs(float(compute_seg_loss(g["warped1"], g["ref_seg"], g["mask1"])) - float(g["per_view"][0])) < 2e-6


def test_segdff_retries_only_failed_items_and_gives_up(monkeypatch):
    """With ops.nmf_solve patched to report a non-finite W for one batch item on the first call: one solve (and one status
    read) for the batch, one re-solve for that item alone; and an error after the attempt limit when every call reports it."""
    from mvs_amd.jdacs.models import seg_dff as M
    calls = []

    def fake(fail_always):
        def nmf_solve(V, W0, H0, update_h=True, max_iter=50, tol=1e-4):
            P = V.shape[0]
            calls.append(P)
            st = torch.zeros(P, 4)
            st[:, 0] = max_iter
            if fail_always or len(calls) == 1:
                st[1 if P > 1 else 0, 1] = 3.0
            return W0 * float(len(calls)), H0, st
        return nmf_solve
    net = S.StandInNet(seed=1)
    imgs = torch.rand(3, 2, 3, 16, 16, generator=torch.Generator().manual_seed(0))
    monkeypatch.setattr(M.ops, "nmf_solve", fake(False))
    heat = M.SegDFF(4, max_iter=5, net=net)(imgs)
    assert calls == [3, 1] and tuple(heat.shape) == (3, 2, 14, 14, 4)
    calls.clear()
    monkeypatch.setattr(M.ops, "nmf_solve", fake(True))
    with pytest.raises(RuntimeError, match="after %d attempts" % M.MAX_ATTEMPTS):
        M.SegDFF(4, max_iter=5, net=net)(imgs)
    assert calls == [3] + [1] * (M.MAX_ATTEMPTS - 1)


def test_segdff_without_torchvision_says_so(monkeypatch):
    import sys
    from mvs_amd.jdacs.models.seg_dff import SegDFF
    monkeypatch.setitem(sys.modules, "torchvision", None)       # import torchvision -> ImportError
    with pytest.raises(ImportError, match="torchvision"):
        SegDFF(4)


def test_nmf_dropin_signature(emul_lib):
    """NMF(V, k, ...) returns (W, H) like the reference: seeded factors from a private generator; a caller-supplied H stays."""
    from mvs_amd.jdacs.models.seg_dff import NMF
    c = nmf_case("g15_nmf_small", "fixedh_")
    W, H = NMF(c["V"], 4, H=c["H0"].clone(), random_seed=None, max_iter=c["max_iter"], tol=c["tol"], W=c["W0"].clone())
    assert torch.equal(H, c["H0"]) and float((W - c["W"]).abs().max()) <= 2e-5 * float(c["W"].abs().max())
    e = nmf_case("g15_nmf_small", "early_")
    V = e["V"][:96, :40].contiguous()
    W1, H1 = NMF(V, 4, random_seed=7, max_iter=11, cuda=False)
    W2, H2 = NMF(V, 4, random_seed=7, max_iter=11, cuda=False)
    assert torch.equal(W1, W2) and torch.equal(H1, H2) and tuple(W1.shape) == (96, 4) and tuple(H1.shape) == (4, 40)
    W0, H0 = S.nmf_initial_factors(V, 4, 7)
    Wo, _, _, _, _, _ = S.nmf_iterate(V.double(), W0, H0, True, 11, 1e-4)
    assert float((W1 - Wo).abs().max()) <= 2e-5 * float(Wo.abs().max())


def test_aug_loss_and_random_image_mask_vs_reference_fixture(emul_lib):
    from mvs_amd.jdacs.models.augmentations import aug_loss, random_image_mask
    from mvs_amd.jdacs_ms.models import augmentations as A2
    assert A2.aug_loss is aug_loss and A2.random_image_mask is random_image_mask
    g = load_golden("g15_aug")
    np.random.seed(int(g["np_seed"]))
    masked, fmask = random_image_mask(g["img"], tuple(int(x) for x in g["filter_size"]))
    assert torch.equal(masked, g["masked"]) and torch.equal(fmask, g["filter_mask"])
    same, none = random_image_mask(g["img"], tuple(g["img"].shape[2:]))
    assert none is None and same is g["img"]
    est = g["est"].clone().requires_grad_(True)
    loss = aug_loss(est, g["gt"], fmask[:, 0])
    (3.0 * loss).backward()
    assert abs(float(loss) - float(g["loss"])) < 2e-6 * abs(float(g["loss"]))
    assert float((est.grad - g["grad_est_x3"]).abs().max()) <= 1e-5 * float(g["grad_est_x3"].abs().max())


def _product_lib():
    from mvs_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.MvsLib()


def test_new_entry_points_reject_bad_arguments():
    """mvs_nmf_* / mvs_seg_loss_*: null pointers and every limit are rejected on the host before any launch, with a message;
    the workspace queries answer -1 for the same shapes and the documented sizes otherwise (product library, no GPU needed)."""
    lib = _product_lib()
    d = C.c_void_p(64)                      # never dereferenced
    ok = (2, 64, 32, 4)
    nmf = lambda V=d, W=d, H=d, shape=ok, upd=1, it=10, tol=1e-4, ws=d, st=d: lib.call(
        "mvs_nmf_solve", V, W, H, *shape, upd, it, tol, ws, st, None)
    for kw in ({"V": None}, {"W": None}, {"H": None}, {"ws": None}, {"st": None}):
        with pytest.raises(ValueError, match="null pointer"):
            nmf(**kw)
    bad_shapes = [((0, 64, 32, 4), "P >= 1"), ((1, 64, 32, 0), "1 <= k <= 8"), ((1, 64, 32, 9), "1 <= k <= 8"),
                  ((1, 3, 32, 4), "n >= k and m >= k"), ((1, 64, 3, 4), "n >= k and m >= k"), ((1, 65536, 32768, 4), "2\\^31")]
    for shape, msg in bad_shapes:
        with pytest.raises(ValueError, match=msg):
            nmf(shape=shape)
        assert lib.raw("mvs_nmf_workspace_floats", *shape) == -1, shape
    with pytest.raises(ValueError, match="max_iter"):
        nmf(it=0)
    with pytest.raises(ValueError, match="tol is NaN"):
        nmf(tol=float("nan"))
    for P, n, m, k in ((1, 1372, 512, 4), (4, 320, 96, 3), (1, 8, 8, 8), (2, 17, 5, 1)):
        nblk = (n + 15) // 16
        assert lib.raw("mvs_nmf_workspace_floats", P, n, m, k) == P * (16 + n * k + nblk * k * m + nblk * k * k + nblk * 2)
    assert lib.raw("mvs_nmf_workspace_floats", 1, 65536, 32767, 4) > 0

    views = (C.c_void_p * 11)(*([64] * 11))
    seg = lambda ref=d, vs=views, kinv=d, proj=d, depth=d, shape=(2, 4, 16, 20, 4), ws=d: (ref, vs, kinv, proj, depth) + shape + (ws,)
    for kw in ({"ref": None}, {"vs": None}, {"kinv": None}, {"proj": None}, {"depth": None}, {"ws": None}):
        with pytest.raises(ValueError, match="null pointer"):
            lib.call("mvs_seg_loss_fwd", *seg(**kw), d, None)
        with pytest.raises(ValueError, match="null pointer"):
            lib.call("mvs_seg_loss_bwd", *seg(**kw), d, d, None)
    holes = (C.c_void_p * 4)(64, 64, None, 64)
    with pytest.raises(ValueError, match="null view map 2"):
        lib.call("mvs_seg_loss_fwd", *seg(vs=holes), d, None)
    with pytest.raises(ValueError, match="null output"):
        lib.call("mvs_seg_loss_fwd", *seg(), None, None)
    with pytest.raises(ValueError, match="null gradient"):
        lib.call("mvs_seg_loss_bwd", *seg(), None, d, None)
    with pytest.raises(ValueError, match="null gradient"):
        lib.call("mvs_seg_loss_bwd", *seg(), d, None, None)
    bad_shapes = [((1, 0, 8, 8, 4), "1 <= V <= 10"), ((1, 11, 8, 8, 4), "1 <= V <= 10"), ((1, 4, 8, 8, 1), "2 <= K <= 8"),
                  ((1, 4, 8, 8, 9), "2 <= K <= 8"), ((0, 4, 8, 8, 4), "B >= 1"), ((1, 4, 1, 8, 4), "H >= 2 and W >= 2"),
                  ((1, 4, 8, 1, 4), "H >= 2 and W >= 2"), ((16, 4, 8192, 4096, 4), "2\\^31")]
    for shape, msg in bad_shapes:
        with pytest.raises(ValueError, match=msg):
            lib.call("mvs_seg_loss_fwd", *seg(shape=shape), d, None)
        with pytest.raises(ValueError, match=msg):
            lib.call("mvs_seg_loss_bwd", *seg(shape=shape), d, d, None)
        assert lib.raw("mvs_seg_loss_workspace_floats", *shape) == -1, shape
    for b, v, h, w, k in ((2, 4, 32, 40, 4), (1, 1, 2, 2, 2), (4, 6, 128, 160, 4), (1, 10, 27, 35, 8)):
        assert lib.raw("mvs_seg_loss_workspace_floats", b, v, h, w, k) == 2 * v * ((b * h * w + 255) // 256) + 16
    assert lib.launch_trace() == []


def test_new_sources_enqueue_only():
    """The new C sources hold no stream / device / event synchronisation and no device-to-host copy: the solve and the loss
    are enqueued and return (the GPU suite checks the same at run time under torch's sync-debug mode)."""
    src = open(os.path.join(ROOT, "self-supervised-mvs_amd", "csrc", "seg_loss_kernels.h")).read()
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("Synchronize", "hipMemcpy", "hipStreamQuery", "hipEventQuery", "hipHostMalloc", "hipStreamWaitEvent"):
        assert word not in code, word
    assert "mvs_nmf_solve" in code and "mvs_seg_loss_bwd" in code
    # and nothing waits on another workgroup: no atomics, no spinning on memory
    for word in ("atomic", "while (", "volatile", "__threadfence"):
        assert word not in code, word
