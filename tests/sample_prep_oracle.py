"""TEST-SIDE restatement, in torch and parametrised by dtype (float32 / float64), of the arithmetic of training-sample preparation
(csrc/sample_prep_kernels.h, include/mvs_hip.h): torchvision's tensor formulas of ColorJitter's four operations, the reference's
RandomGamma.adjust_gamma(clip_image=True), center_image, ToTensor + ImageNet Normalize, random_image_mask's window and its nearest
F.interpolate(scale_factor=0.25).  Also the seeded cases the CPU-emulation and the GPU tests share."""
import itertools

import numpy as np
import torch

SEG_MEAN = (0.485, 0.456, 0.406)
SEG_STD = (0.229, 0.224, 0.225)
ORDERS = list(itertools.permutations(range(4)))         # the 24 application orders of the four operations


def gray(x):
    """x [..., 3] -> [...]"""
    return 0.299 * x[..., 0] + 0.587 * x[..., 1] + 0.114 * x[..., 2]


def brightness(x, f):
    return (f * x).clamp(0, 1)


def contrast(x, f):
    return (f * x + (1 - f) * gray(x).mean()).clamp(0, 1)


def saturation(x, f):
    return (f * x + (1 - f) * gray(x).unsqueeze(-1)).clamp(0, 1)


def hue(x, f):
    """rgb -> hsv, h = (h + f) mod 1, hsv -> rgb with colorsys's conventions; a grey pixel has s = 0 and h = 0 (no division by 0)"""
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    maxc, minc = x.max(-1).values, x.min(-1).values
    d = maxc - minc
    grey = d == 0
    one, zero = torch.ones((), dtype=x.dtype, device=x.device), torch.zeros((), dtype=x.dtype, device=x.device)
    sd, sm = torch.where(grey, one, d), torch.where(grey, one, maxc)
    s = torch.where(grey, zero, d / sm)
    rc, gc, bc = (maxc - r) / sd, (maxc - g) / sd, (maxc - b) / sd
    h = torch.where(r == maxc, bc - gc, torch.where(g == maxc, 2 + rc - bc, 4 + gc - rc)) / 6
    h = h - torch.floor(h)
    h = torch.where(grey, zero, h)
    h = h + f
    h = h - torch.floor(h)
    v = maxc
    h6 = h * 6
    i = torch.floor(h6)
    ff = h6 - i
    p, q, t = v * (1 - s), v * (1 - s * ff), v * (1 - s * (1 - ff))
    i = i.long() % 6
    pick = lambda *six: torch.stack(six, 0).gather(0, i.unsqueeze(0))[0]
    out = torch.stack([pick(v, q, p, p, t, v), pick(t, v, v, q, p, p), pick(p, p, t, v, v, q)], dim=-1)
    return torch.where(grey.unsqueeze(-1), x, out)


OPS = (brightness, contrast, saturation, hue)


def chain(u8_img, row, dtype):
    """u8_img [H, W, 3] uint8, row: the view's 9 parameters -> the jittered, gamma-corrected image [H, W, 3] in [0, 1]"""
    x = u8_img.to(dtype) / 255
    scalar = lambda v: torch.tensor(float(v), dtype=dtype, device=x.device)       # the table's fp32 value, exactly
    for k in range(4):
        op = int(row[k])
        if op >= 0:
            x = OPS[op](x, scalar(row[4 + k]))
    return torch.pow(x, scalar(row[8])).clamp(0, 1)


def center_image(x):
    """x [H, W, 3]: (x - mean) / (sqrt(var) + 1e-8), population statistics per channel"""
    var = x.var(dim=(0, 1), unbiased=False, keepdim=True)
    mean = x.mean(dim=(0, 1), keepdim=True)
    return (x - mean) / (var.sqrt() + 1e-8)


def quantise(x):
    """fp32 [M, 3, H, W] in [0, 1] -> uint8 [M, H, W, 3] as ToPILImage does: x255, truncate"""
    return (x * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def window_mask(rect, H, W, dtype, device=None):
    m = torch.ones(H, W, dtype=dtype, device=device)
    y, x, fh, fw = (int(v) for v in rect)
    if fh > 0:
        m[y:y + fh, x:x + fw] = 0
    return m


def prepare(u8, table, rects, dtype, aug_center=True, mask_scale=None):
    """u8 [M, H, W, 3] -> dict of "imgs", "imgs_aug" (with a table), "imgs_seg" [M, 3, H, W] and "filter_mask" [M, H // s, W // s]"""
    M, H, W, _ = u8.shape
    out = {"imgs": [], "imgs_seg": []}
    if table is not None:
        out["imgs_aug"] = []
    if mask_scale is not None:
        out["filter_mask"] = []
    mean, std = torch.tensor(SEG_MEAN, dtype=dtype, device=u8.device), torch.tensor(SEG_STD, dtype=dtype, device=u8.device)
    for m in range(M):
        raw = u8[m].to(dtype)
        out["imgs"].append(center_image(raw))
        out["imgs_seg"].append((raw / 255 - mean) / std)
        wm = window_mask(rects[m] if rects is not None else (0, 0, 0, 0), H, W, dtype, u8.device)
        if table is not None:
            x = chain(u8[m], table[m], dtype)
            if aug_center:
                x = center_image(x * 255)
            out["imgs_aug"].append(x * wm.unsqueeze(-1))
        if mask_scale is not None:
            out["filter_mask"].append(wm[::mask_scale, ::mask_scale][:H // mask_scale, :W // mask_scale])
    res = {}
    for k, v in out.items():
        v = torch.stack(v, 0)
        res[k] = v if k == "filter_mask" else v.permute(0, 3, 1, 2).contiguous()
    return res


def check_outputs(ours, o32, o64, what=""):
    """The criteria of the issue: imgs within 1e-6 max|truth| of the fp64 evaluation (exact integer statistics: one fp32
    rounding); imgs_aug and imgs_seg as accurate as the fp32 evaluation is; filter_mask exactly equal."""
    from conftest import assert_as_accurate_as_fp32_reference
    assert set(ours) == set(o64), (sorted(ours), sorted(o64))
    for k, v in ours.items():
        assert v.shape == o64[k].shape and v.dtype == torch.float32, (what, k, tuple(v.shape), tuple(o64[k].shape))
        if k == "imgs":
            err, top = float((v.double() - o64[k]).abs().max()), float(o64[k].abs().max())
            print("%s imgs: max err %.3e, 1e-6 max|truth| %.3e" % (what, err, 1e-6 * top))
            assert err <= 1e-6 * top, "%s imgs max err %.3e vs %.3e" % (what, err, 1e-6 * top)
        elif k == "filter_mask":
            assert torch.equal(v, o64[k].float()), what + " filter_mask"
        else:
            print("%s %s: max err %.3e, fp32 oracle's %.3e" % (what, k, float((v - o64[k].float()).abs().max()),
                                                              float((o32[k] - o64[k].float()).abs().max())))
            assert_as_accurate_as_fp32_reference(v, o32[k], o64[k], what=what + " " + k)


# ---- seeded cases shared by tests/test_sample_prep.py (emulated kernels) and tests/test_gpu_sample_prep.py -------------------------

def seeded_views(M, H, W, seed):
    """uint8 [M, H, W, 3]: smooth colour ramps plus noise, with black, white, grey and fully saturated pixels in every view"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    views = []
    for m in range(M):
        ph = torch.rand(3, generator=g) * 6.28
        base = torch.stack([127 + 100 * torch.sin(0.11 * (m + 1) * xx + 0.07 * yy + ph[c]) for c in range(3)], dim=-1)
        img = (base + 40 * torch.randn(H, W, 3, generator=g)).clamp(0, 255).to(torch.uint8)
        flat = img.view(-1, 3)
        special = torch.tensor([[0, 0, 0], [255, 255, 255], [128, 128, 128], [255, 0, 0], [0, 255, 0], [0, 0, 255], [7, 7, 7],
                                [255, 255, 0]], dtype=torch.uint8)
        n = min(len(special), flat.shape[0])
        idx = torch.randperm(flat.shape[0], generator=g)[:n]
        flat[idx] = special[:n]
        views.append(img)
    return torch.stack(views, 0)


def seeded_table(M, seed, first_order=0, gammas=(0.5, 1.0, 2.0), absent=()):
    """fp32 [M, 9]: view m applies the four operations in ORDERS[(first_order + m) % 24] with factors uniform in the loaders'
    ranges (brightness, contrast [0, 2], saturation [0.5, 1.5], hue [-0.5, 0.5]); gamma cycles through `gammas`, then is uniform in
    [0.5, 2]; in the views listed in `absent` the second and the fourth position are absent (-1)."""
    rs = np.random.RandomState(seed)
    lo, hi = (0.0, 0.0, 0.5, -0.5), (2.0, 2.0, 1.5, 0.5)
    table = np.empty((M, 9), np.float32)
    for m in range(M):
        order = ORDERS[(first_order + m) % 24]
        for k, op in enumerate(order):
            table[m, k], table[m, 4 + k] = op, rs.uniform(lo[op], hi[op])
        table[m, 8] = gammas[m] if m < len(gammas) else rs.uniform(0.5, 2.0)
        if m in absent:
            table[m, [1, 3]] = -1
    return table


def seeded_rects(M, H, W, N, seed, frac=3):
    """int32 [M, 4]: an (H // frac, W // frac) window on the first of every N views, none on the others"""
    rs = np.random.RandomState(seed)
    rects = np.zeros((M, 4), np.int32)
    fh, fw = H // frac, W // frac
    if fh < 1 or fw < 1:
        return rects
    for m in range(0, M, N):
        x = rs.randint(0, W - fw)
        y = rs.randint(0, H - fh)
        rects[m] = (y, x, fh, fw)
    return rects


# name -> (M, H, W, rows used, views per sample); the shapes of the issue: smaller than a tile; odd pixel count, unaligned image
# offsets, H / 4 and W / 4 floored; several tiles; a ragged last tile with W no multiple of 16; a 32-row crop read through the image
# stride; and 24 small views, one per operation order
CASES = {
    "tiny": (1, 5, 7, 5, 1),
    "odd": (3, 37, 53, 37, 3),
    "tiles": (5, 128, 160, 128, 5),
    "ragged": (2, 130, 1030, 130, 2),
    "crop": (2, 40, 48, 32, 2),
    "orders": (24, 9, 11, 9, 3),
}


def make_case(name):
    """-> (stored uint8 views [M, H, W, 3], the views the kernel is to use (a row-prefix slice for "crop"), table, rects)"""
    M, H, W, rows, N = CASES[name]
    seed = 700 + 10 * sorted(CASES).index(name)
    stored = seeded_views(M, H, W, seed)
    used = stored[:, :rows]
    first = {"tiny": 5, "odd": 7, "tiles": 11, "ragged": 17, "crop": 21, "orders": 0}[name]
    absent = {"tiles": (1, 3), "odd": (2,)}.get(name, ())
    table = seeded_table(M, seed + 1, first_order=first, absent=absent)
    if name == "tiles":
        table[4, 4 + list(table[4, :4]).index(3.0)] = 0.5          # hue shifts of exactly +0.5 and -0.5
        table[2, 4 + list(table[2, :4]).index(3.0)] = -0.5
    rects = seeded_rects(M, rows, W, N, seed + 2)
    return stored, used, table, rects


def augmentor_case():
    """fp32 [2 * 3, 3, 36, 52] in [0, 1] whose x255 is k + 0.5 (so the truncation does not depend on the last bit), with exact 0 and
    1 among them; brightness and contrast only, one order and one pair of factors per sample of three views, a gamma per view; an
    (h // 4, w // 4) window on the first view of each sample"""
    M, H, W = 6, 36, 52
    u8 = seeded_views(M, H, W, 790)
    x = ((u8.float() + 0.5) / 255).clamp(0, 1).permute(0, 3, 1, 2).contiguous()
    x[u8.permute(0, 3, 1, 2) == 0] = 0.0
    x[u8.permute(0, 3, 1, 2) == 255] = 1.0
    rs = np.random.RandomState(791)
    table = np.full((M, 9), -1, np.float32)
    table[:, 4:8] = 1.0
    for b in range(2):
        order = (0, 1) if b == 0 else (1, 0)
        f = rs.uniform(0.5, 1.5, size=2)
        for n in range(3):
            table[3 * b + n, :2] = order
            table[3 * b + n, 4:6] = f
            table[3 * b + n, 8] = rs.uniform(0.7, 2.0)
    rects = seeded_rects(M, H, W, 3, 792, frac=4)
    return x, table, rects
