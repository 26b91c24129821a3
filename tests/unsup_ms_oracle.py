"""TEST INFRASTRUCTURE: the jdacs-ms UnSupLoss (jdacs-ms/losses/unsup_loss.py:18-82) composed from the oracle's primitives.

The jdacs-ms loss is the jdacs one at full image resolution (no 0.25x down-sampling; images only permuted to NHWC), with the
smoothness weight 0.05 and lambda 1.0.  Pinned to the reference by tests/golden/g14_unsup_loss_ms*.npz."""
import torch

from oracle import ref_torch as R

W_RECONSTR, W_SSIM, W_SMOOTH, SMOOTH_LAMBDA = 12.0, 6.0, 0.05, 1.0


def unsup_loss_ms(imgs, cams, depth, return_terms=False):
    """imgs [B,N,3,H,W], cams [B,N,2,4,4] (full-resolution intrinsics), depth [B,H,W] -> total (, reconstr, ssim, smooth)."""
    n = imgs.shape[1]
    ref = imgs[:, 0].permute(0, 2, 3, 1)
    vols, ssim = [], 0.0
    for v in range(1, n):
        kinv, proj = R.unsup_view_transform(cams[:, 0], cams[:, v])
        warped, mask = R.unsup_inverse_warp(imgs[:, v].permute(0, 2, 3, 1), kinv, proj, depth)
        vols.append(R.unsup_reconstr_term(warped, ref, mask) + 1e4 * (1 - mask))
        if v < 3:
            ssim = ssim + R.unsup_ssim_map(ref, warped, mask).mean()
    smooth = R.unsup_smoothness(depth, ref, SMOOTH_LAMBDA)
    vol = torch.stack(vols).permute(1, 2, 3, 4, 0)
    top = -torch.topk(-vol, k=3, sorted=False)[0]
    top = top * (top < 1e4).float()
    reconstr = top.sum(-1).mean()
    total = W_RECONSTR * reconstr + W_SSIM * ssim + W_SMOOTH * smooth
    return (total, reconstr, ssim, smooth) if return_terms else total


def synthetic_ms_inputs(b, n, h, w, seed, depth_mean=640.0):
    """Smooth random images [B,N,3,H,W], cameras [B,N,2,4,4] with full-resolution intrinsics (batch items differ), depth [B,H,W]."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(seed)
    imgs = F.avg_pool2d(torch.randn(b * n, 3, h, w, generator=gen), 5, 1, 2).view(b, n, 3, h, w) * 3
    K, E = R.synthetic_cameras(n, h, w, w)
    cams = torch.zeros(b, n, 2, 4, 4)
    cams[:, :, 0] = E
    cams[:, :, 1, :3, :3] = K
    cams[1:, 1:, 0, :3, 3] *= 1.2
    depth = depth_mean + 40.0 * torch.rand(b, h, w, generator=gen)
    return imgs, cams, depth
