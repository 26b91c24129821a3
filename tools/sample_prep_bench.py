#!/usr/bin/env python3
"""Timing evidence for training-sample preparation on one GPU, at B = 1 with N = 3 and N = 5 views of 512 x 640 (the training
crops) and N = 5 views of 1184 x 1600 (jdacs-ms's full size):
  (a) SamplePrep / ops.sample_prep: the three launches of csrc/sample_prep_kernels.h from the uint8 views, nothing read back;
  (b) the same arithmetic written here with stock PyTorch-ROCm ops on the same GPU, from the same uint8 views: per view the four
      jitter operations in the view's order (hue through hsv as torchvision's tensor path does), gamma, x255, center_image, the
      window, plus center_image of the raw view, ToTensor + Normalize and the strided mask;
  (c) where PIL is importable: the reference's host path for ONE view (PIL ImageEnhance / HSV hue, ToTensor, gamma, two
      center_image, Normalize) in milliseconds of CPU time per view, for orientation only.
(a) and (b) are timed with torch.cuda.Event pairs after 8 warm-up runs, one pair per repetition, 40 repetitions; reported are the
median and the 10th / 90th percentiles.  Also counted per call: kernel launches ((a) from the library's launch trace, both from the
torch profiler) and host synchronisations (torch's sync-debug mode "warn").

    python tools/sample_prep_bench.py [--size NAME]

One size per process keeps every GPU step under a limit of its own:
    timeout -k 10 240 python tools/sample_prep_bench.py --size n3_512x640 && \\
    timeout -k 10 240 python tools/sample_prep_bench.py --size n5_512x640 && \\
    timeout -k 10 300 python tools/sample_prep_bench.py --size n5_1184x1600
Each run adds its size to profiles/sample_prep_timing.json and prints the file's content."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import mvs_amd  # noqa: F401
from mvs_amd import _lib
from mvs_amd.sample_prep import SamplePrep

REPS, WARMUP = 40, 8
SIZES = {"n3_512x640": (3, 512, 640), "n5_512x640": (5, 512, 640), "n5_1184x1600": (5, 1184, 1600)}
OUT = os.path.join(ROOT, "profiles", "sample_prep_timing.json")
dev = torch.device("cuda:0")


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    q = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]
    return {"median_ms": q(0.5), "p10_ms": q(0.1), "p90_ms": q(0.9), "reps": REPS, "warmup": WARMUP}


def profiled_launches(fn):
    """device kernels + memsets + copies one call enqueues, counted by the torch profiler (None where it is unavailable)"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
    except Exception as exc:  # noqa: BLE001
        sys.stderr.write("launch count unavailable: %r\n" % (exc,))
        return None


def host_syncs(fn):
    fn()
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return sum(1 for w in caught if "synchroniz" in str(w.message).lower() and "prototype feature" not in str(w.message))


# ---- (b) the same arithmetic with stock ops ------------------------------------------------------------------------------------------

def _gray(x):
    return 0.299 * x[0] + 0.587 * x[1] + 0.114 * x[2]


def _hue(x, f):
    r, g, b = x[0], x[1], x[2]
    maxc, minc = x.max(0).values, x.min(0).values
    d = maxc - minc
    grey = d == 0
    sd, sm = torch.where(grey, torch.ones_like(d), d), torch.where(grey, torch.ones_like(d), maxc)
    s = torch.where(grey, torch.zeros_like(d), d / sm)
    rc, gc, bc = (maxc - r) / sd, (maxc - g) / sd, (maxc - b) / sd
    h = torch.where(r == maxc, bc - gc, torch.where(g == maxc, 2 + rc - bc, 4 + gc - rc)) / 6
    h = torch.where(grey, torch.zeros_like(d), h - torch.floor(h)) + f
    h = h - torch.floor(h)
    h6 = h * 6
    i = torch.floor(h6)
    ff = h6 - i
    v = maxc
    p, q, t = v * (1 - s), v * (1 - s * ff), v * (1 - s * (1 - ff))
    i = (i.long() % 6).unsqueeze(0)
    pick = lambda *six: torch.stack(six, 0).gather(0, i)[0]
    return torch.stack([pick(v, q, p, p, t, v), pick(t, v, v, q, p, p), pick(p, p, t, v, v, q)], 0)


def _center(x):
    var, mean = x.var(dim=(1, 2), unbiased=False, keepdim=True), x.mean(dim=(1, 2), keepdim=True)
    return (x - mean) / (var.sqrt() + 1e-8)


def stock_ops(views, table, rects, seg_mean, seg_std):
    """views uint8 [N, H, W, 3] on the device; table, rects host arrays -> the four tensors, with stock ops only"""
    N, H, W, _ = views.shape
    imgs, augs, segs = [], [], []
    for n in range(N):
        raw = views[n].permute(2, 0, 1).float()
        imgs.append(_center(raw))
        x = raw / 255
        segs.append((x - seg_mean) / seg_std)
        for k in range(4):
            op, f = int(table[n, k]), float(table[n, 4 + k])
            if op == 0:
                x = (f * x).clamp(0, 1)
            elif op == 1:
                x = (f * x + (1 - f) * _gray(x).mean()).clamp(0, 1)
            elif op == 2:
                x = (f * x + (1 - f) * _gray(x)).clamp(0, 1)
            elif op == 3:
                x = _hue(x, f)
        x = _center(torch.pow(x, float(table[n, 8])).clamp(0, 1) * 255)
        y0, x0, fh, fw = (int(v) for v in rects[n])
        if fh > 0:
            x[:, y0:y0 + fh, x0:x0 + fw] = 0
        augs.append(x)
    mask = torch.ones(H // 4, W // 4, device=views.device)
    y0, x0, fh, fw = (int(v) for v in rects[0])
    mask[(y0 + 3) // 4:(y0 + fh + 3) // 4, (x0 + 3) // 4:(x0 + fw + 3) // 4] = 0          # the pixels (4 i, 4 j) inside the window
    return torch.stack(imgs), torch.stack(augs), torch.stack(segs), mask


# ---- (c) the reference's host path for one view ---------------------------------------------------------------------------------------

def pil_one_view(u8, row):
    from PIL import Image, ImageEnhance
    img = Image.fromarray(u8, "RGB")
    raw = u8.astype(np.float32)
    imgs = (raw - raw.mean((0, 1), keepdims=True)) / (np.sqrt(raw.var((0, 1), keepdims=True)) + 1e-8)
    for k in range(4):
        op, f = int(row[k]), float(row[4 + k])
        if op == 0:
            img = ImageEnhance.Brightness(img).enhance(f)
        elif op == 1:
            img = ImageEnhance.Contrast(img).enhance(f)
        elif op == 2:
            img = ImageEnhance.Color(img).enhance(f)
        elif op == 3:                                      # torchvision's PIL adjust_hue
            h, s, v = img.convert("HSV").split()
            nh = ((np.array(h, dtype=np.int32) + int(f * 255)) % 256).astype(np.uint8)          # uint8 wrap-around
            img = Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB")
    x = torch.from_numpy(np.asarray(img).astype(np.float32) / 255)
    x = (torch.pow(x, float(row[8])).clamp_(0, 1) * 255).numpy()
    aug = (x - x.mean((0, 1), keepdims=True)) / (np.sqrt(x.var((0, 1), keepdims=True)) + 1e-8)
    seg = (raw / 255 - np.asarray([0.485, 0.456, 0.406], np.float32)) / np.asarray([0.229, 0.224, 0.225], np.float32)
    return imgs, aug, seg


def views_of(N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    out = []
    for n in range(N):
        base = torch.stack([127 + 100 * torch.sin(0.011 * (n + 1) * xx + 0.007 * yy + c) for c in range(3)], dim=-1)
        out.append((base + 30 * torch.randn(H, W, 3, generator=g)).clamp(0, 255).to(torch.uint8))
    return torch.stack(out)


def run_size(name):
    N, H, W = SIZES[name]
    lib = _lib.get()
    views = views_of(N, H, W, 900 + N).to(dev)
    prep, rs = SamplePrep(), np.random.RandomState(17)
    table, win = prep.draw(N, rs), prep.window(1, H, W, (H // 3, W // 3), rs)
    rects = np.zeros((N, 4), np.int32)
    rects[0] = win[0]
    seg_mean = torch.tensor([0.485, 0.456, 0.406], device=dev).view(3, 1, 1)
    seg_std = torch.tensor([0.229, 0.224, 0.225], device=dev).view(3, 1, 1)
    batch = views.view(1, N, H, W, 3)

    def ours():
        return prep(batch, table, win)

    def stock():
        return stock_ops(views, table, rects, seg_mean, seg_std)

    a, b = ours(), stock()
    diff = {"imgs": float((a["imgs"][0] - b[0]).abs().max()), "imgs_aug": float((a["imgs_aug"][0] - b[1]).abs().max()),
            "imgs_seg": float((a["imgs_seg"][0] - b[2]).abs().max()), "filter_mask": float((a["filter_mask"][0] - b[3]).abs().max())}
    lib.launch_trace()
    ours()
    trace = lib.launch_trace()
    row = {"N": N, "H": H, "W": W, "a_sample_prep": timed(ours), "b_stock_ops": timed(stock),
           "a_library_launches": len(trace), "a_launch_trace": trace,
           "profiled_launches": {"a_sample_prep": profiled_launches(ours), "b_stock_ops": profiled_launches(stock)},
           "host_syncs": {"a_sample_prep": host_syncs(ours), "b_stock_ops": host_syncs(stock)},
           "max_abs_difference_a_vs_b": diff,
           "bytes": {"u8_read_per_pass": N * H * W * 3, "fp32_written": 3 * N * H * W * 3 * 4 + (H // 4) * (W // 4) * 4 * N}}
    row["ratio_b_over_a_median"] = row["b_stock_ops"]["median_ms"] / row["a_sample_prep"]["median_ms"]
    try:
        import PIL  # noqa: F401
        u8 = views[0].cpu().numpy()
        pil_one_view(u8, table[0])
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            pil_one_view(u8, table[0])
            t.append((time.perf_counter() - t0) * 1e3)
        row["c_pil_host_ms_per_view"] = {"min_of_3": min(t), "views": N, "per_sample_ms": min(t) * N}
    except ImportError:
        row["c_pil_host_ms_per_view"] = None
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", choices=sorted(SIZES), default=None, help="one size (default: all three, in this process)")
    args = ap.parse_args()
    res = {"what": "training-sample preparation from uint8 views: (a) SamplePrep (csrc/sample_prep_kernels.h), (b) the same arithmetic "
                   "with stock PyTorch-ROCm ops on the same GPU, (c) the reference's PIL host path per view (CPU, orientation only)",
           "sizes": {}}
    if os.path.exists(OUT):
        with open(OUT) as fh:
            res = json.load(fh)
    res["device"] = torch.cuda.get_device_name(0)
    for name in ([args.size] if args.size else list(SIZES)):
        res["sizes"][name] = run_size(name)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
