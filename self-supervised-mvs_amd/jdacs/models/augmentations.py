"""The two functions of jdacs/models/augmentations.py the training step calls besides the torchvision-style colour transforms
(train.py:246,277): ``random_image_mask`` and ``aug_loss``.  ``aug_loss`` -- boolean-mask gathers + smooth-L1 in the
reference -- is the one-launch masked smooth-L1 kernel (ops.MaskedSmoothL1, csrc/loss.hip)."""
import numpy as np
import torch

from ... import ops


def random_image_mask(img, filter_size):
    """img [B,3,H,W] -> (img with a random fh x fw window zeroed, the mask); (img, None) when the window is the whole image.
    The window's corner comes from ``np.random`` (x first, then y), as in the reference (augmentations.py:107-125)."""
    fh, fw = filter_size
    _, _, h, w = img.size()
    if fh == h and fw == w:
        return img, None
    x = np.random.randint(0, w - fw)
    y = np.random.randint(0, h - fh)
    filter_mask = torch.ones_like(img)
    filter_mask[:, :, y:y + fh, x:x + fw] = 0.0
    return img * filter_mask, filter_mask


def aug_loss(depth_est, depth_gt, mask):
    """mean smooth-L1 of depth_est - depth_gt over mask > 0.5 (augmentations.py:128-130); differentiable w.r.t. depth_est."""
    return ops.MaskedSmoothL1.apply(depth_est, depth_gt, mask)
