"""Drop-in for jdacs-ms/losses/unsup_loss.py: ``UnSupLoss()(imgs, cams, depth)``.

Same constructor (no arguments), call signature, value and attributes after a call (``reconstr_loss``, ``ssim_loss``,
``smooth_loss``, ``unsup_loss``) as the reference class (unsup_loss.py:18-82).  Unlike the jdacs loss it works at full image
resolution on the depth map that train.py nearest-up-samples to the image size (train.py:222-229), with the weights
12 / 6 / 0.05 and smoothness lambda 1.0.  The reference's per-view indexing / elementwise launches and its index_put backward
are five HIP launches forward and two backward (csrc/unsup_loss.hip, mvs_unsup_loss_weighted_*)."""
import torch
import torch.nn as nn

from ... import ops
from ...jdacs.losses.unsup_loss import less_one_percentage, less_three_percentage, non_zero_mean_absolute_diff  # noqa: F401  (:89-128, the same text as jdacs)


class UnSupLoss(nn.Module):
    W_RECONSTR, W_SSIM, W_SMOOTH = 12.0, 6.0, 0.05     # unsup_loss.py:82
    SMOOTH_LAMBDA = 1.0                               # unsup_loss.py:69

    def __init__(self):
        super().__init__()

    def forward(self, imgs, cams, depth):
        """imgs [B,N,3,H,W], cams [B,N,2,4,4] (extrinsic, intrinsic at image resolution; float32 or float64), depth [B,H,W]."""
        if imgs.dim() != 5 or cams.dim() != 5 or imgs.shape[1] != cams.shape[1]:
            raise ValueError("Different number of images and projection matrices: imgs %s cams %s"
                             % (tuple(imgs.shape), tuple(cams.shape)))
        b, n, _, h, w = imgs.shape
        if n < 4:
            raise ValueError("UnSupLoss selects the 3 best of the N-1 source views (unsup_loss.py:71-76): needs N >= 4, got "
                             "imgs %s" % (tuple(imgs.shape),))
        if tuple(depth.shape) != (b, h, w):
            raise ValueError("depth must be [B,H,W] at image resolution = %s, got %s (imgs %s)"
                             % ((b, h, w), tuple(depth.shape), tuple(imgs.shape)))
        with torch.no_grad():
            # one permute to [N,B,H,W,3]: every view a contiguous NHWC image (unsup_loss.py:36,53)
            x = imgs.detach().float().permute(1, 0, 3, 4, 2).contiguous()
            kinv, proj = ops.unsup_view_transforms(cams.detach().float())
        total, reconstr, ssim, smooth = ops.unsup_loss_weighted(depth, x[0], [x[v] for v in range(1, n)], kinv, proj,
                                                                self.W_RECONSTR, self.W_SSIM, self.W_SMOOTH,
                                                                self.SMOOTH_LAMBDA)
        self.reconstr_loss, self.ssim_loss, self.smooth_loss = reconstr, ssim, smooth
        self.unsup_loss = total
        return total
