"""Training-sample preparation on the device: from the decoded uint8 views of a batch to the tensors ``train_sample`` /
``train_sample_aug`` of both reference trees consume (``imgs``, ``imgs_aug``, ``imgs_seg`` and the ``filter_mask`` of the
augmentation-consistency branch).

The reference's loaders do this per view on the host (jdacs/datasets/dtu_yao.py:59-67, 94-99, 231-247, 279-281;
jdacs-ms/dataset/dtu.py:80-86, 112-119, 164-166, 207-219): ``center_image`` of the raw view, PIL ``ColorJitter(1, 1, 0.5, 0.5)``
-> ``ToTensor`` -> ``RandomGamma(0.5, 2.0, clip)`` -> x255 -> ``center_image`` for the augmented one, ``ToTensor`` -> ImageNet
``Normalize`` for the segmentation branch; train.py then zeroes a random window of the augmented reference view and shrinks its
mask by 4 (jdacs/train.py:269-275).  Here the loader hands over the uint8 views only; the random parameters are drawn on the host
(``draw``, ``window``) and ``ops.sample_prep`` (csrc/sample_prep_kernels.h) computes everything in three launches.
"""
import numpy as np
import torch

from . import ops

OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE, OP_NONE = 0, 1, 2, 3, -1


def _range(value, center=1.0, lo_bound=0.0):
    """torchvision's ColorJitter._check_input: a number v -> [max(lo_bound, center - v), center + v]; a zero setting (or a pair
    that collapses on the centre) means the operation is absent."""
    if isinstance(value, (tuple, list)):
        lo, hi = float(value[0]), float(value[1])
    else:
        value = float(value)
        if value < 0:
            raise ValueError("a jitter setting must be non-negative, got %r" % (value,))
        lo, hi = center - value, center + value
        if lo_bound is not None:
            lo = max(lo, lo_bound)
    if lo > hi:
        raise ValueError("empty jitter range [%g, %g]" % (lo, hi))
    return None if lo == hi == center else (lo, hi)


class SamplePrep:
    """``prep = SamplePrep(); out = prep(views_u8, prep.draw(B * N, rng), prep.window(B, H, W, (H // 3, W // 3), rng))``.

    brightness, contrast, saturation: a number v for factors in [max(0, 1 - v), 1 + v]; hue: h for shifts in [-h, h] (h <= 0.5);
    gamma: (min, max).  seg: also return ``imgs_seg``.  mask_scale: 4 gives the ``filter_mask`` of train.py:274-275, 1 the
    full-size one.  The defaults are the loaders' of both trees."""

    def __init__(self, brightness=1, contrast=1, saturation=0.5, hue=0.5, gamma=(0.5, 2.0), seg=True, mask_scale=4,
                 channels_last=False):
        self.ranges = (_range(brightness), _range(contrast), _range(saturation), _range(hue, center=0.0, lo_bound=None))
        if self.ranges[3] is not None and not (-0.5 <= self.ranges[3][0] and self.ranges[3][1] <= 0.5):
            raise ValueError("hue shifts must stay within [-0.5, 0.5], got %r" % (self.ranges[3],))
        self.gamma = (float(gamma[0]), float(gamma[1]))
        if not 0.0 < self.gamma[0] <= self.gamma[1]:
            raise ValueError("gamma range must be positive and ordered, got %r" % (gamma,))
        self.seg = bool(seg)
        self.mask_scale = mask_scale
        self.channels_last = bool(channels_last)

    def draw(self, M, rng, group=1):
        """The parameter table fp32 [M, 9] of M views: four operation ids in application order (-1 behind the present ones),
        their factors, gamma.  Per jitter draw, as ColorJitter.get_params: the factors of the present operations in the order
        brightness, contrast, saturation, hue, each uniform in its range, then a uniform permutation of them; then, per view, gamma
        uniform in its range as RandomGamma.get_params.  group: views that share one jitter draw (Augmentor: the N views of a
        sample); their gammas are drawn one after the other behind it.  rng: a numpy.random.RandomState."""
        if M % group:
            raise ValueError("draw: M = %d is no multiple of group = %d" % (M, group))
        table = np.empty((M, 9), np.float32)
        for g0 in range(0, M, group):
            ids, factors = [], []
            for op, r in enumerate(self.ranges):
                if r is not None:
                    ids.append(op)
                    factors.append(rng.uniform(r[0], r[1]))
            order = rng.permutation(len(ids)) if ids else []
            row = [float(OP_NONE)] * 4 + [1.0] * 4
            for k, j in enumerate(order):
                row[k], row[4 + k] = float(ids[j]), factors[j]
            for m in range(g0, g0 + group):
                table[m, :8] = row
                table[m, 8] = rng.uniform(self.gamma[0], self.gamma[1])
        return table

    @staticmethod
    def window(B, H, W, filter_size, rng, per_sample=False):
        """The windows int32 [B, 4] = (y, x, fh, fw) that random_image_mask zeroes: x = randint(0, W - fw) first, then y =
        randint(0, H - fh) (jdacs/models/augmentations.py:120-121).  One draw serves the whole batch, as the reference's call on
        the batched reference view does; per_sample draws one per sample.  A window of the whole image is no window (the reference
        returns the image unchanged and no mask): all zeros."""
        fh, fw = int(filter_size[0]), int(filter_size[1])
        rects = np.zeros((B, 4), np.int32)
        if fh == H and fw == W:
            return rects
        for b in range(B if per_sample else 1):
            x = rng.randint(0, W - fw)
            y = rng.randint(0, H - fh)
            rects[b] = (y, x, fh, fw)
        if not per_sample:
            rects[:] = rects[0]
        return rects

    def __call__(self, views_u8, table, rects=None, rows=None):
        """views_u8 [B, N, H, W, 3] uint8 on the device; table [B * N, 9] from ``draw`` (None: no ``imgs_aug``); rects [B, 4] from
        ``window`` for the reference view of each sample (None: no window, no ``filter_mask``).  rows: use the first ``rows`` image
        rows only, read in place (jdacs-ms's center_image crops 1200 to 1184).  Returns {"imgs", "imgs_aug", "imgs_seg"}
        [B, N, 3, H, W] and "filter_mask" [B, H // s, W // s]."""
        if views_u8.dim() != 5 or views_u8.shape[4] != 3 or views_u8.dtype != torch.uint8:
            raise ValueError("SamplePrep: views must be uint8 [B, N, H, W, 3], got %s %s" % (views_u8.dtype, tuple(views_u8.shape)))
        B, N, H, W = views_u8.shape[:4]
        flat = views_u8.reshape(B * N, H, W, 3)
        if rows is not None:
            if not 1 <= rows <= H:
                raise ValueError("SamplePrep: rows = %r outside 1..%d" % (rows, H))
            flat, H = flat[:, :rows], rows
        view_rects = None
        if rects is not None:
            rects = np.asarray(rects, np.int32)
            if rects.shape != (B, 4):
                raise ValueError("SamplePrep: rects must be [B = %d, 4], got %s" % (B, rects.shape))
            view_rects = np.zeros((B, N, 4), np.int32)
            view_rects[:, 0] = rects
            view_rects = view_rects.reshape(B * N, 4)
        out = ops.sample_prep(flat, table, view_rects, imgs=True, seg=self.seg,
                              mask_scale=self.mask_scale if rects is not None else None, aug_center=True,
                              channels_last=self.channels_last)
        res = {}
        for k, v in out.items():
            res[k] = v.view(B, N, *v.shape[1:])[:, 0] if k == "filter_mask" else v.view(B, N, 3, H, W)
        return res
