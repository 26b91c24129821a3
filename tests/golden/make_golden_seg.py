#!/usr/bin/env python3
"""Generate tests/golden/g15_*.npz by IMPORTING the reference's co-segmentation code (build container only).

    python tests/golden/make_golden_seg.py

`jdacs/models/seg_dff.py` imports torchvision at module level (for the pretrained VGG19 only); an empty stand-in module is
registered under that name, which is enough for `NMF`, `compute_seg_loss`, `inverse_warping` and `UnSupSegLoss.forward` to load
and run on the CPU.  Only arrays are stored: seeded inputs (V as 8-bit multiples of 1/32, images / maps / cameras / depths as
float16-exact values), the reference's factors, iteration counts, loss terms and gradients.

Three conditions on the INPUTS are asserted (another seed is taken otherwise), so that no comparison hinges on one rounding:
  1. every stopping test the reference evaluates is at least a factor 1.2 away from `tol`, in fp32 and in fp64;
  2. no pixel's source coordinate lies within 1e-3 px of an integer that decides its validity;
  3. the two largest values of ref_seg are at least 1e-4 apart at every pixel.
The fp32 restatement of the iteration in tests/seg_oracle.py is asserted to reproduce the reference's NMF bit for bit here."""
import os
import sys
import types
import warnings

sys.dont_write_bytecode = True
warnings.filterwarnings("ignore")
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import seg_oracle as S  # noqa: E402  (input generators, conditions and the restated iteration)

REF = "/root/reference"
sys.argv = ["x"]
sys.path.insert(0, os.path.join(REF, "jdacs"))
_tv = types.ModuleType("torchvision")
_tv.models = types.ModuleType("torchvision.models")
sys.modules["torchvision"] = _tv
sys.modules["torchvision.models"] = _tv.models


class _Names(types.ModuleType):
    """every name resolves to `object`: enough for the class statements of jdacs/models/augmentations.py to execute"""
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return object


_tv.transforms = _Names("torchvision.transforms")
sys.modules["torchvision.transforms"] = _tv.transforms
torch.set_num_threads(4)
from models.seg_dff import NMF  # noqa: E402
from losses.unsup_seg_loss import UnSupSegLoss  # noqa: E402
from losses.homography import inverse_warping  # noqa: E402
from models.augmentations import aug_loss, random_image_mask  # noqa: E402


def quantised(V):
    """V as multiples of 1/32 in [0, 255/32]: stored as uint8"""
    q = torch.clamp(torch.round(V * 32.0), 0, 255)
    return q / 32.0, q.to(torch.uint8).numpy()


def nmf_case(prefix, out, n, m, k, seed, tol=1e-4, max_iter=50, zero=0, fixed_h=False, want_iters=None, noise=0.3):
    for attempt in range(400):
        s = seed + 100 * attempt
        V, Vq = quantised(S.relu_like_matrix(n, m, k, s, zero, zero, noise))
        W0, H0 = S.nmf_initial_factors(V, k, s)
        if fixed_h:                                    # a caller-supplied H: the reference draws W only and keeps H
            Hg = H0.clone()
            Wr, Hr = NMF(V.clone(), k, H=Hg.clone(), random_seed=s, max_iter=max_iter, tol=tol, cuda=False)
        else:
            Wr, Hr = NMF(V.clone(), k, random_seed=s, max_iter=max_iter, tol=tol, cuda=False)
        W32, H32, it32, t32, e0, elast = S.nmf_iterate(V, W0, H0, not fixed_h, max_iter, tol)
        W64, H64, it64, t64, _, _ = S.nmf_iterate(V.double(), W0, H0, not fixed_h, max_iter, tol)
        assert torch.equal(W32, Wr) and torch.equal(H32, Hr), "the restated iteration does not reproduce the reference bit for bit"
        if S.stopping_tests_clear_of_tol(t32, tol) and S.stopping_tests_clear_of_tol(t64, tol) and it32 == it64 and \
                (want_iters is None or it32 == want_iters):
            break
    else:
        raise RuntimeError("no seed meets the stopping-test condition for " + prefix)
    if zero:
        assert int((V.sum(1) == 0).sum()) >= zero and int((V.sum(0) == 0).sum()) >= zero
        assert bool((Wr[V.sum(1) == 0] == 0).all()) and bool((Hr[:, V.sum(0) == 0] == 0).all())
    out.update({prefix + "Vq": Vq, prefix + "W0": W0.numpy(), prefix + "H0": H0.numpy(), prefix + "W": Wr.numpy(), prefix + "H": Hr.numpy(),
                prefix + "iters": np.int32(it32), prefix + "tol": np.float32(tol), prefix + "max_iter": np.int32(max_iter),
                prefix + "update_h": np.int32(0 if fixed_h else 1), prefix + "e0": np.float32(e0), prefix + "e_last": np.float32(elast),
                prefix + "tests": np.asarray(t32, np.float32)})
    print("%-12s n=%d m=%d k=%d seed %d: %d iterations, tests %s (fp64 %s), fp32-vs-fp64 W %.2e of max" % (
        prefix, n, m, k, s, it32, ["%.3e" % t for t in t32], ["%.3e" % t for t in t64],
        float((W32 - W64).abs().max() / W64.abs().max())))


class _Maps(nn.Module):
    """stands in for SegDFF inside the reference's UnSupSegLoss: returns the given maps"""
    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, imgs):
        return self.fn(imgs)


def reference_seg_loss(seg_fn, imgs, cams, depth):
    crit = UnSupSegLoss.__new__(UnSupSegLoss)
    nn.Module.__init__(crit)
    crit.seg_model = _Maps(seg_fn)
    return crit(imgs, cams, depth)


def seg_case(name, b, n, h, w, s, k, seed):
    seg, cams, depth = S.synthetic_seg_inputs(b, n, h, w, s, k, seed)
    assert S.seg_inputs_well_conditioned(seg, cams, depth)
    d = depth.clone().requires_grad_(True)
    total, ref_seg, view_segs = reference_seg_loss(lambda imgs: seg, None, cams, d)
    total.backward()
    with torch.no_grad():
        terms = []
        for v in range(1, n):
            warped, mask = inverse_warping(view_segs[:, v - 1], cams[:, 0], cams[:, v], depth)
            from losses.unsup_seg_loss import compute_seg_loss
            terms.append(compute_seg_loss(warped, ref_seg, mask))
            if v == 1:
                warped1, mask1 = warped, mask
    out = dict(seg=seg.half().numpy(), cams=cams.numpy(), depth=depth.numpy(), loss=total.detach().numpy(),
               per_view=torch.stack(terms).numpy(), ref_seg=ref_seg.detach().numpy(), view_segs=view_segs.detach().numpy(),
               warped1=warped1.numpy(), mask1=mask1.numpy(), grad_depth=d.grad.numpy())
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print("%-20s %7.1f KB  loss %.6f terms %s valid %.2f |grad| max %.3e" % (
        name, os.path.getsize(path) / 1024, float(total), ["%.5f" % float(t) for t in terms], float(mask1.mean()),
        float(d.grad.abs().max())))


def e2e_case(name, b, n, h, w, k, seed):
    """images -> stand-in network -> the reference's NMF per batch item (SegDFF.forward's steps with cuda=False) -> the
    reference's UnSupSegLoss.forward."""
    net = S.StandInNet(seed=3)
    for attempt in range(50):
        g = torch.Generator().manual_seed(seed + 1000 * attempt)
        low = torch.randn(b * n, 3, 6, 8, generator=g)
        imgs = (F.interpolate(low, size=(4 * h, 4 * w), mode="bicubic", align_corners=False)
                + 0.1 * torch.randn(b * n, 3, 4 * h, 4 * w, generator=g)).view(b, n, 3, 4 * h, 4 * w).half().float()
        _, cams, depth = S.synthetic_seg_inputs(b, n, h, w, 4, k, seed + attempt)

        def seg_fn(x):
            maps = []
            for i in range(x.size(0)):
                with torch.no_grad():
                    xi = F.interpolate(x[i], size=(224, 224), mode="bilinear", align_corners=False)
                    f = net.features(xi)
                    flat = f.permute(0, 2, 3, 1).contiguous().view(-1, f.size(1))
                    W, _ = NMF(flat, k, random_seed=1, cuda=False, max_iter=50, verbose=False)
                    assert not bool(torch.isnan(W).any())
                    maps.append(W.view(f.size(0), f.size(2), f.size(3), k))
            return torch.stack(maps, 0)
        heat = seg_fn(imgs)
        flat_ok = True
        for i in range(b):                             # condition 1 on the problems this case solves
            xi = F.interpolate(imgs[i], size=(224, 224), mode="bilinear", align_corners=False)
            f = net.features(xi).detach()
            flat = f.permute(0, 2, 3, 1).contiguous().view(-1, f.size(1))
            W0, H0 = S.nmf_initial_factors(flat, k, 1)
            W32, _, i32, t32, _, _ = S.nmf_iterate(flat, W0, H0, True, 50, 1e-4)
            _, _, i64, t64, _, _ = S.nmf_iterate(flat.double(), W0, H0, True, 50, 1e-4)
            assert torch.equal(W32.view_as(heat[i]), heat[i])
            flat_ok &= S.stopping_tests_clear_of_tol(t32, 1e-4) and S.stopping_tests_clear_of_tol(t64, 1e-4) and i32 == i64
        if flat_ok and S.seg_inputs_well_conditioned(heat, cams, depth):
            break
    else:
        raise RuntimeError("no well-conditioned end-to-end inputs")
    d = depth.clone().requires_grad_(True)
    total, ref_seg, view_segs = reference_seg_loss(seg_fn, imgs, cams, d)
    total.backward()
    out = dict(imgs=imgs.half().numpy(), cams=cams.numpy(), depth=depth.numpy(), heatmaps=heat.numpy(), loss=total.detach().numpy(),
               ref_seg=ref_seg.detach().numpy(), view_segs=view_segs.detach().numpy(), grad_depth=d.grad.numpy(),
               net_seed=np.int32(3), K=np.int32(k))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print("%-20s %7.1f KB  loss %.6f |grad| max %.3e" % (name, os.path.getsize(path) / 1024, float(total), float(d.grad.abs().max())))


small = {}
nmf_case("ragged_", small, 320, 96, 4, 11, zero=5)
nmf_case("k3_", small, 200, 64, 3, 12)
nmf_case("early_", small, 240, 80, 4, 13, tol=5e-2, want_iters=11, noise=0.6)      # noisier data: stops after iteration 10
nmf_case("fixedh_", small, 200, 64, 4, 14, max_iter=21, fixed_h=True)
np.savez_compressed(os.path.join(HERE, "g15_nmf_small.npz"), **small)
train = {}
nmf_case("train_", train, 7 * 14 * 14, 512, 4, 15)
np.savez_compressed(os.path.join(HERE, "g15_nmf_train.npz"), **train)
for f in ("g15_nmf_small.npz", "g15_nmf_train.npz"):
    print("%-20s %7.1f KB" % (f, os.path.getsize(os.path.join(HERE, f)) / 1024))
seg_case("g15_seg_loss", 2, 5, 32, 40, 6, 4, 21)
seg_case("g15_seg_loss_odd", 1, 2, 27, 35, 5, 3, 22)
e2e_case("g15_seg_e2e", 2, 3, 16, 20, 4, 23)


def aug_case(name):
    """random_image_mask with np.random.seed(5) and aug_loss with its gradient, on seeded float16-exact inputs"""
    g = torch.Generator().manual_seed(41)
    img = torch.randn(2, 3, 24, 32, generator=g).half().float()
    np.random.seed(5)
    masked, fmask = random_image_mask(img, (6, 8))
    whole, none = random_image_mask(img, (24, 32))
    assert none is None and whole is img
    est = (600.0 + 3.0 * torch.randn(2, 24, 32, generator=g)).half().float().requires_grad_(True)
    gt = (600.0 + 3.0 * torch.randn(2, 24, 32, generator=g)).half().float()
    loss = aug_loss(est, gt, fmask[:, 0])
    (3.0 * loss).backward()
    np.savez_compressed(os.path.join(HERE, name + ".npz"), img=img.half().numpy(), masked=masked.numpy(), filter_mask=fmask.numpy(),
                        est=est.detach().numpy(), gt=gt.numpy(), loss=loss.detach().numpy(), grad_est_x3=est.grad.numpy(),
                        np_seed=np.int32(5), filter_size=np.asarray([6, 8], np.int32))
    print("%-20s loss %.6f window zeros %d" % (name, float(loss), int((fmask == 0).sum())))


aug_case("g15_aug")
