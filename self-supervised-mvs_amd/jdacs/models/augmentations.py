"""jdacs/models/augmentations.py: ``random_image_mask`` and ``aug_loss`` (train.py:246,277), and the device-side augmentation
module ``Augmentor`` with its ``get_transform`` / ``RandomGamma`` (augmentations.py:20-104).  ``aug_loss`` -- boolean-mask gathers
+ smooth-L1 in the reference -- is the one-launch masked smooth-L1 kernel (ops.MaskedSmoothL1, csrc/loss.hip).  The colour
transforms -- a ToPILImage / PIL ColorJitter / ToTensor / gamma round trip through the host per view in the reference -- are
ops.sample_prep (csrc/sample_prep_kernels.h) on the tensors where they are; the random parameters are drawn on the host from
``np.random`` (mvs_amd.sample_prep.SamplePrep.draw)."""
import numpy as np
import torch
import torch.nn as nn

from ... import ops
from ...sample_prep import SamplePrep


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


class RandomGamma():
    """augmentations.py:68-92: a gamma per image, uniform in [min_gamma, max_gamma] from ``np.random``.  ``adjust_gamma`` is the
    reference's definition on whatever tensor it is given (a loader's host-side transform); on the device the same formula is the
    last step of ops.sample_prep's chain."""

    def __init__(self, min_gamma=0.7, max_gamma=1.5, clip_image=False):
        self._min_gamma = min_gamma
        self._max_gamma = max_gamma
        self._clip_image = clip_image

    @staticmethod
    def get_params(min_gamma, max_gamma):
        return np.random.uniform(min_gamma, max_gamma)

    @staticmethod
    def adjust_gamma(image, gamma, clip_image):
        adjusted = torch.pow(image, gamma)
        if clip_image:
            adjusted.clamp_(0.0, 1.0)
        return adjusted

    def __call__(self, imgs):
        res = []
        for im in imgs:
            gamma = self.get_params(self._min_gamma, self._max_gamma)
            res.append(self.adjust_gamma(im, gamma, self._clip_image))
        return res


class _ViewsTransform:
    """What get_transform() returns: the chain ToPILImage -> ColorJitter(0.5, 0.5, 0, 0) -> ToTensor -> RandomGamma(0.7, 2.0, clip)
    of augmentations.py:42-48 on the views of ONE sample: one jitter draw shared by the views, a gamma per view, no centring."""

    def __init__(self):
        self.prep = SamplePrep(brightness=0.5, contrast=0.5, saturation=0, hue=0, gamma=(0.7, 2.0), seg=False)

    def draw(self, B, N):
        return self.prep.draw(B * N, np.random.mtrand._rand, group=N)

    def __call__(self, imgs):
        """imgs: the N views [3,H,W] in [0,1] of one sample (a list, or a tensor [N,3,H,W]) -> list of N tensors [3,H,W]"""
        views = imgs if isinstance(imgs, torch.Tensor) else torch.stack(list(imgs), dim=0)
        out = ops.sample_prep(views, self.draw(1, views.shape[0]), None, imgs=False, seg=False, aug_center=False)["imgs_aug"]
        return list(out.unbind(0))


def get_transform():
    return _ViewsTransform()


class Augmentor(nn.Module):
    """augmentations.py:20-39: imgs [B,N,3,H,W] in [0,1] -> (augmented imgs, filter_mask [B,3,H,W]).  Brightness and contrast 0.5,
    ONE jitter draw per sample shared by its views, a gamma in [0.7, 2.0] per view, no centring; then random_image_mask with an
    (h // 4, w // 4) window on the reference view of the batch.  The whole batch is one ops.sample_prep call (two launches).  The
    mask's three channels are one plane expanded (a view: clone it before writing into it)."""

    def __init__(self):
        super(Augmentor, self).__init__()
        self.transform = get_transform()

    def forward(self, imgs):
        if imgs.dim() != 5 or imgs.shape[2] != 3:
            raise ValueError("Augmentor: imgs must be [B,N,3,H,W], got %s" % (tuple(imgs.shape),))
        B, N, _, h, w = imgs.shape
        rng = np.random.mtrand._rand
        table = self.transform.draw(B, N)
        rects = np.zeros((B, N, 4), np.int32)
        rects[:, 0] = SamplePrep.window(B, h, w, (h // 4, w // 4), rng)
        out = ops.sample_prep(imgs.reshape(B * N, 3, h, w), table, rects.reshape(B * N, 4), imgs=False, seg=False, mask_scale=1,
                              aug_center=False)
        filter_mask = out["filter_mask"].view(B, N, 1, h, w)[:, 0].expand(B, 3, h, w)
        return out["imgs_aug"].view(B, N, 3, h, w), filter_mask
