"""Drop-in for jdacs/losses/unsup_seg_loss.py: ``UnSupSegLoss(args)(imgs, cams, depth)``.

Same call signature and return triple (reproj_seg_loss, ref_seg [B,H,W,K], view_segs [B,V,H,W,K]) as the reference class
(unsup_seg_loss.py:37-80).  The per-view ``inverse_warping`` + boolean-mask gathers + ``F.cross_entropy`` of the reference
are two HIP launches forward and one backward for all views (csrc/seg_loss_kernels.h); the two bilinear up-samplings of the
segmentation maps to the depth resolution stay ``F.interpolate``, one call for all views."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from ..models.seg_dff import SegDFF


def compute_seg_loss(warped_seg, ref_seg, mask):
    """Plain torch, for callers that use it on its own: mean cross-entropy of the warped maps [B,H,W,K] against the arg-max of
    ref_seg over the pixels with mask [B,H,W,1] > 0.5."""
    k = warped_seg.size(3)
    sel = mask.repeat(1, 1, 1, k) > 0.5
    logits = warped_seg[sel].contiguous().view(-1, k)
    target = torch.argmax(ref_seg[sel].contiguous().view(-1, k), dim=1)
    return F.cross_entropy(logits, target)


class UnSupSegLoss(nn.Module):
    def __init__(self, args_or_K, net=None, hip_features=None, feature_arith="f32"):
        """args_or_K: the reference's ``args`` (its ``seg_clusters`` is used) or the number of clusters K; net: SegDFF's
        feature extractor (None: the pretrained VGG19); hip_features, feature_arith: SegDFF's, passed through unchanged."""
        super().__init__()
        k = args_or_K if isinstance(args_or_K, int) else args_or_K.seg_clusters
        self.seg_model = SegDFF(K=k, max_iter=50, net=net, hip_features=hip_features, feature_arith=feature_arith)

    def forward(self, imgs, cams, depth):
        """imgs [B,N,3,H,W], cams [B,N,2,4,4] (intrinsics at the depth map's resolution), depth [B,h,w]."""
        if imgs.dim() != 5 or cams.dim() != 5 or imgs.shape[1] != cams.shape[1]:
            raise ValueError("Different number of images and projection matrices: imgs %s cams %s"
                             % (tuple(imgs.shape), tuple(cams.shape)))
        b, n = imgs.shape[:2]
        if n < 2:
            raise ValueError("UnSupSegLoss needs at least one source view: N >= 2, got %d" % n)
        seg_maps = self.seg_model(imgs)                       # [B,N,s,s,K]
        height, width = depth.size(1), depth.size(2)
        with torch.no_grad():
            s1, s2, k = seg_maps.shape[2:]
            up = F.interpolate(seg_maps.permute(0, 1, 4, 2, 3).reshape(b * n, k, s1, s2), size=(height, width), mode='bilinear')
            up = up.permute(0, 2, 3, 1).reshape(b, n, height, width, k)
            kinv, proj = ops.unsup_view_transforms(cams.float())
        ref_seg, view_segs = up[:, 0], up[:, 1:]
        total, per_view = ops.seg_loss(depth, ref_seg, [view_segs[:, v] for v in range(n - 1)], kinv, proj)
        self.reprojection_losses = per_view
        return total, ref_seg, view_segs
