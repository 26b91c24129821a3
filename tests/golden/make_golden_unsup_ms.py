#!/usr/bin/env python3
"""Generate tests/golden/g14_unsup_loss_ms*.npz by IMPORTING the reference's jdacs-ms UnSupLoss (build container only).

    python tests/golden/make_golden_unsup_ms.py

`jdacs-ms/losses/unsup_loss.py` loads on the CPU without argv or config handling.  The loss runs at full image resolution
(jdacs-ms/train.py:222-229 up-samples every level's depth map to the image size first), so the cameras carry full-resolution
intrinsics.  Only tensors are stored: seeded inputs (images as float16-exact values), the loss, its three terms, the gradient
w.r.t. the depth map and the first view's warped image + mask."""
import os
import sys
import warnings

sys.dont_write_bytecode = True
warnings.filterwarnings("ignore")
import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle.ref_torch import synthetic_cameras  # shared synthetic camera definition (inputs only)

REF = "/root/reference"
sys.argv = ["x"]
sys.path.insert(0, os.path.join(REF, "jdacs-ms"))
torch.set_num_threads(4)
from losses.unsup_loss import UnSupLoss  # noqa: E402
from losses.homography import inverse_warping  # noqa: E402


def textured_images(b, n, h, w, g):
    """smooth random textures (so that the photometric terms have a usable gradient), float16-exact"""
    low = torch.randn(b * n, 3, max(h // 8, 2), max(w // 8, 2), generator=g)
    img = F.interpolate(low, size=(h, w), mode="bicubic", align_corners=False) + 0.1 * torch.randn(b * n, 3, h, w, generator=g)
    return img.view(b, n, 3, h, w).half().float()


def make(name, b, n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    imgs = textured_images(b, n, h, w, g)
    K, E = synthetic_cameras(n, h, w, w)
    cams = torch.zeros(b, n, 2, 4, 4)
    cams[:, :, 0] = E
    cams[:, :, 1, :3, :3] = K
    cams[1:, 1:, 0, :3, 3] *= 1.3           # batch items differ
    cams = cams.half().float()
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    depth = (640.0 + 0.4 * xx - 0.5 * yy + 6.0 * torch.randn(b, h, w, generator=g)).half().float()
    depth = depth.clone().requires_grad_(True)
    crit = UnSupLoss()
    loss = crit(imgs, cams, depth)
    loss.backward()
    with torch.no_grad():
        warped1, mask1 = inverse_warping(imgs[:, 1].permute(0, 2, 3, 1), cams[:, 0], cams[:, 1], depth.detach())
    out = dict(imgs=imgs.half().numpy(), cams=cams.numpy(), depth=depth.detach().numpy(), loss=loss.detach().numpy(),
               reconstr_loss=crit.reconstr_loss.detach().numpy(), ssim_loss=crit.ssim_loss.detach().numpy(),
               smooth_loss=crit.smooth_loss.detach().numpy(), grad_depth=depth.grad.numpy(),
               warped1=warped1.numpy(), mask1=mask1.numpy())
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print("%-26s %7.1f KB  loss %.6f (reconstr %.6f ssim %.6f smooth %.6f) valid %.2f |grad| %.3e" % (
        name, os.path.getsize(path) / 1024, float(loss), float(crit.reconstr_loss), float(crit.ssim_loss),
        float(crit.smooth_loss), float(mask1.mean()), float(depth.grad.abs().mean())))


make("g14_unsup_loss_ms", 2, 7, 48, 64, 31)
make("g14_unsup_loss_ms_n4", 1, 4, 45, 61, 32)
