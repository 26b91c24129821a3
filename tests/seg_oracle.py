"""TEST INFRASTRUCTURE: the JDACS co-segmentation loss restated for the tests -- the NMF iteration of jdacs/models/seg_dff.py:21-106
(dtype-generic, returning the value of every stopping test) and UnSupSegLoss.forward (jdacs/losses/unsup_seg_loss.py:21-80) composed
from the oracle's warp primitives.  Pinned to the reference by tests/golden/g15_*.npz (tests/golden/make_golden_seg.py)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import ref_torch as R

EPSILON = 1e-7


def nmf_initial_factors(V, k, seed):
    """|randn| * sqrt(mean(V) / k), W drawn before H, from a generator seeded with `seed` (seg_dff.py:55-89 on the CPU)."""
    g = torch.Generator().manual_seed(seed)
    scale = torch.sqrt(V.float().mean() / k)
    W = torch.randn(V.shape[0], k, generator=g) * scale
    H = torch.randn(k, V.shape[1], generator=g) * scale
    return W.abs(), H.abs()


def nmf_iterate(V, W0, H0, update_h=True, max_iter=50, tol=1e-4):
    """The reference's iteration op for op in V's dtype.  -> W, H, iterations run, [stopping-test values], e0, last e."""
    V = V.clone()
    W, H = W0.to(V.dtype).clone(), H0.to(V.dtype).clone()
    e0 = torch.norm(V - torch.mm(W, H))
    prev, last, tests = e0, e0, []
    VH = HH = None
    it = 0
    for it in range(max_iter):
        if VH is None:
            Ht = torch.t(H)
            VH = torch.mm(V, Ht)
            HH = torch.mm(H, Ht)
        WHH = torch.mm(W, HH)
        WHH[WHH == 0] = EPSILON
        W *= VH / WHH
        if update_h:
            Wt = torch.t(W)
            WV = torch.mm(Wt, V)
            WWH = torch.mm(torch.mm(Wt, W), H)
            WWH[WWH == 0] = EPSILON
            H *= WV / WWH
            VH = HH = None
        if tol > 0 and it % 10 == 0:
            last = torch.norm(V - torch.mm(W, H))
            tests.append(float((prev - last) / e0))
            if (prev - last) / e0 < tol:
                break
            prev = last
    return W, H, it + 1, tests, float(e0), float(last)


def relu_like_matrix(n, m, rank, seed, zero_rows=0, zero_cols=0, noise=0.3):
    """V = relu(A B + noise) >= 0 as float16-exact values (what a ReLU feature map looks like), optionally with all-zero rows / columns."""
    g = torch.Generator().manual_seed(seed)
    V = torch.relu(torch.rand(n, rank, generator=g) @ torch.rand(rank, m, generator=g) - 0.25 * rank * 0.5
                   + noise * torch.randn(n, m, generator=g))
    if zero_rows:
        V[torch.randperm(n, generator=g)[:zero_rows]] = 0
    if zero_cols:
        V[:, torch.randperm(m, generator=g)[:zero_cols]] = 0
    return V.half().float()


def stopping_tests_clear_of_tol(tests, tol, factor=1.2):
    """Input condition of the fixtures: no stopping test within a factor 1.2 of the tolerance."""
    return all(t >= factor * tol or t <= tol / factor for t in tests)


# ---- segmentation loss ------------------------------------------------------------------------------------------------------
def maps_at_depth_resolution(seg, h, w):
    """seg [B,N,s,s,K] -> ref_seg [B,h,w,K], view_segs [B,N-1,h,w,K] (unsup_seg_loss.py:45-55,63-65)."""
    b, n, s1, s2, k = seg.shape
    up = F.interpolate(seg.permute(0, 1, 4, 2, 3).reshape(b * n, k, s1, s2), size=(h, w), mode="bilinear")
    up = up.permute(0, 2, 3, 1).reshape(b, n, h, w, k)
    return up[:, 0], up[:, 1:]


def inverse_warp_channels(view_seg, kinv, proj, depth):
    """R.unsup_inverse_warp (3 channels) applied to groups of three of the K channels: the bilinear gather is per channel."""
    k = view_seg.shape[-1]
    pad = (-k) % 3
    x = torch.cat([view_seg, view_seg[..., :1].expand(*view_seg.shape[:-1], pad)], -1) if pad else view_seg
    outs, mask = [], None
    for c in range(0, k + pad, 3):
        o, mask = R.unsup_inverse_warp(x[..., c:c + 3], kinv, proj, depth)
        outs.append(o)
    return torch.cat(outs, -1)[..., :k], mask


def compute_seg_loss(warped_seg, ref_seg, mask):
    """unsup_seg_loss.py:21-34."""
    k = warped_seg.size(3)
    sel = mask.repeat(1, 1, 1, k) > 0.5
    logits = warped_seg[sel].contiguous().view(-1, k)
    target = torch.argmax(ref_seg[sel].contiguous().view(-1, k), dim=1)
    return F.cross_entropy(logits, target)


def seg_loss(seg, cams, depth, return_parts=False):
    """seg [B,N,s,s,K] (SegDFF's output), cams [B,N,2,4,4], depth [B,h,w] -> total (, per-view terms, ref_seg, view_segs, first
    view's warped map and mask)."""
    h, w = depth.shape[1:]
    ref_seg, view_segs = maps_at_depth_resolution(seg, h, w)
    terms, first = [], None
    for v in range(view_segs.shape[1]):
        kinv, proj = R.unsup_view_transform(cams[:, 0], cams[:, v + 1])
        warped, mask = inverse_warp_channels(view_segs[:, v], kinv, proj, depth)
        if v == 0:
            first = (warped, mask)
        terms.append(compute_seg_loss(warped, ref_seg, mask))
    total = sum(terms) * 1.0
    return (total, torch.stack(terms), ref_seg, view_segs) + first if return_parts else total


def sample_coordinates(cams, depth, dtype=torch.float64):
    """Source coordinates (x, y) [B,V,h,w] of every reference pixel, as inverse_warping forms them."""
    b, h, w = depth.shape
    cams, depth = cams.to(dtype), depth.to(dtype)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=dtype), torch.arange(w, dtype=dtype), indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(h * w, dtype=dtype)], 0)
    out = []
    for v in range(1, cams.shape[1]):
        kinv, proj = R.unsup_view_transform(cams[:, 0], cams[:, v])
        pc = proj[:, :, :3] @ ((kinv @ pix.unsqueeze(0)) * depth.reshape(b, 1, h * w)) + proj[:, :, 3:4]
        out.append(torch.stack([pc[:, 0] / (pc[:, 2] + 1e-10), pc[:, 1] / (pc[:, 2] + 1e-10)], 1).reshape(b, 2, h, w))
    xy = torch.stack(out, 1)
    return xy[:, :, 0], xy[:, :, 1]


def seg_inputs_well_conditioned(seg, cams, depth, px=1e-3, gap=1e-4):
    """The two input conditions of the seg-loss comparisons: no source coordinate within `px` of an integer that decides its
    validity (x: 0 and w-1; y: 0 and h), and the two largest values of ref_seg at least `gap` apart at every pixel."""
    h, w = depth.shape[1:]
    x, y = sample_coordinates(cams, depth)
    near = ((x.abs() < px) | ((x - (w - 1)).abs() < px) | (y.abs() < px) | ((y - h).abs() < px))
    ref_seg, _ = maps_at_depth_resolution(seg, h, w)
    top = ref_seg.topk(2, dim=-1)[0]
    return (not bool(near.any())) and float((top[..., 0] - top[..., 1]).min()) >= gap


def _cameras(b, n, h, w):
    K, E = R.synthetic_cameras(n, h, w, w)
    cams = torch.zeros(b, n, 2, 4, 4)
    cams[:, :, 0] = E
    cams[:, :, 1, :3, :3] = K
    cams[1:, 1:, 0, :3, 3] *= 1.2
    return cams.half().float()


def _maps_and_depth(b, n, h, w, s, k, seed, depth_mean):
    g = torch.Generator().manual_seed(seed)
    seg = (torch.randn(b, n, s, s, k, generator=g).abs() * 2.0).half().float()
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    depth = (depth_mean + 0.4 * xx - 0.5 * yy + 6.0 * torch.randn(b, h, w, generator=g)).half().float()
    return seg, depth


def coordinates_clear_of_integers(cams, depth, px=1e-3):
    """No source coordinate within `px` of any integer: neither the validity mask nor the bilinear cell (and with it the slope
    that the depth gradient takes) of any pixel hinges on fp32 rounding."""
    x, y = sample_coordinates(cams, depth)
    return not bool((((x - x.round()).abs() < px) | ((y - y.round()).abs() < px)).any())


def synthetic_seg_inputs(b, n, h, w, s, k, seed, depth_mean=640.0):
    """Non-negative maps [B,N,s,s,K] (float16-exact), cameras at the depth map's resolution (batch items differ), depth
    [B,h,w]; seeds are advanced until the two input conditions hold (small shapes: the fixtures)."""
    cams = _cameras(b, n, h, w)
    for attempt in range(50):
        seg, depth = _maps_and_depth(b, n, h, w, s, k, seed + 1000 * attempt, depth_mean)
        if seg_inputs_well_conditioned(seg, cams, depth):
            return seg, cams, depth
    raise RuntimeError("no well-conditioned seg-loss inputs found")


def conditioned_seg_inputs(seg, b, n, h, w, seed, depth_mean=640.0):
    """Cameras and a depth map for GIVEN maps seg [B,N,s,s,K] at a shape where a fresh seed practically never meets the two input
    conditions (128x160: thousands of pixels per validity boundary and per class boundary).  The depth of a pixel whose source
    coordinate lies within 1e-3 px of ANY integer is moved by one depth unit (~0.05 px of parallax) until none is left -- stronger
    than the validity condition, because d warped / d x jumps at every integer coordinate (the bilinear slope changes from one
    cell to the next), so with ~10^5 samples a few pixels within fp32 rounding of an integer would decide a gradient comparison; where
    the two largest classes of ref_seg are closer than 1e-4 the winning one is raised by 0.005..0.025 in the low-resolution cells around the pixel.
    -> seg, cams, depth with seg_inputs_well_conditioned(seg, cams, depth)."""
    cams = _cameras(b, n, h, w)
    _, depth = _maps_and_depth(b, n, h, w, 2, seg.shape[-1], seed, depth_mean)
    for _ in range(50):
        x, y = sample_coordinates(cams, depth)
        near = (((x - x.round()).abs() < 2e-3) | ((y - y.round()).abs() < 2e-3)).any(1)
        if not bool(near.any()):
            break
        depth = depth + near.float()
    assert coordinates_clear_of_integers(cams, depth)
    seg = seg.clone()
    s1, s2 = seg.shape[2:4]
    g = torch.Generator().manual_seed(seed)
    for _ in range(300):
        ref_seg, _ = maps_at_depth_resolution(seg, h, w)
        top, idx = ref_seg.topk(2, dim=-1)
        bad = (top[..., 0] - top[..., 1] < 2e-4).nonzero()
        if len(bad) == 0:
            break
        for bi, yi, xi in bad.tolist():                 # raise the winning class in the low-resolution cells around the pixel
            cy, cx = yi * s1 // h, xi * s2 // w
            seg[bi, 0, max(cy - 1, 0):cy + 2, max(cx - 1, 0):cx + 2, int(idx[bi, yi, xi, 0])] += 0.005 + 0.02 * float(torch.rand(1, generator=g))
    if not seg_inputs_well_conditioned(seg, cams, depth):
        raise RuntimeError("no well-conditioned seg-loss inputs found")
    return seg, cams, depth


class StandInNet(nn.Module):
    """A small frozen stand-in for the VGG19 trunk in tests: `.features` maps [N,3,224,224] to [N,16,14,14] (two strided
    convolutions + ReLU), so SegDFF's n = N * 196, m = 16."""

    def __init__(self, seed=0):
        super().__init__()
        self.features = nn.Sequential(nn.Conv2d(3, 8, 8, 8), nn.ReLU(), nn.Conv2d(8, 16, 2, 2), nn.ReLU())
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_((torch.randn(p.shape, generator=g) * (0.3 if p.dim() > 1 else 0.1)).half().float())
