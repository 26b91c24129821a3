#!/usr/bin/env python3
"""Timing evidence for RefineNet.hip_pass on one GPU: the refine net alone (jdacs/models/mvsnet.py:77-92) through the one-node HIP pass
(ops.RefineNetFn / ops.refine_eval) against the per-block path it replaces (hip_pass = False: F.interpolate, torch.cat, the library's
convolutions, BatchNorm through ops.BnReLUFn / nn.BatchNorm2d), on the same weights and inputs.
  shapes: B = 1, image 512 x 640 -> map 128 x 160 (BASELINE config 2) and 864 x 1152 -> 216 x 288
  modes:  train (zero_grad + forward + backward, batch statistics), frozen (the same under the freeze idiom), eval (no_grad forward)
The image is imgs[:, 0] of a [1,3,3,H,W] tensor, as MVSNet passes it; image and depth both require a gradient in the two training
modes.  Stock and HIP are INTERLEAVED -- one repetition of each per round, torch.cuda.Event pairs around each -- after 8 warm-up
rounds, 40 rounds; reported are the median and the 10th / 90th percentiles.  The rule of DESIGN.md section 7 decides the default per
mode: on only where the HIP pass's p90 is below the stock path's p10 at BOTH shapes.
Writes one JSON object to profiles/refine_timing.json (--out) and prints it."""
import argparse
import json
import os
import sys

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import mvs_amd  # noqa: F401
from mvs_amd.jdacs.models.mvsnet import RefineNet

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_timing.json"))
ap.add_argument("--rounds", type=int, default=40)
ap.add_argument("--warmup", type=int, default=8)
args = ap.parse_args()
ROUNDS, WARMUP = args.rounds, args.warmup
SHAPES = ((512, 640), (864, 1152))
dev = torch.device("cuda:0")
assert torch.cuda.is_available(), "refine_bench measures on the GPU"


def summary(ms):
    ms = sorted(ms)
    q = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]
    return {"median_ms": q(0.5), "p10_ms": q(0.1), "p90_ms": q(0.9), "rounds": ROUNDS, "warmup": WARMUP}


def set_mode(net, mode):
    net.train()
    if mode == "eval":
        net.eval()
    elif mode == "frozen":
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.eval()


def make_step(net, mode, imgs, depth, gout, last, tag):
    def run():
        if mode == "eval":
            with torch.no_grad():
                last[tag] = net(imgs[:, 0], depth)
            return
        net.zero_grad(set_to_none=True)
        imgs.grad = depth.grad = None
        out = net(imgs[:, 0], depth)
        (out * gout).sum().backward()
        last[tag] = out.detach()
    return run


res = {"what": "RefineNet alone, B = 1: stock = RefineNet.hip_pass False (the per-block path), hip = the one-node pass; train / frozen: "
               "zero_grad + forward + backward with image and depth gradients; eval: no_grad forward; interleaved rounds",
       "device": torch.cuda.get_device_name(0), "cases": {}}
wins = {"train": True, "frozen": True, "eval": True}
for H, W in SHAPES:
    g = torch.Generator().manual_seed(H + W)
    h, w = H // 4, W // 4
    imgs = torch.randn(1, 3, 3, H, W, generator=g).to(dev).requires_grad_(True)
    depth = (425.0 + 510.0 * torch.rand(1, h, w, generator=g)).to(dev).requires_grad_(True)
    gout = torch.randn(1, h, w, generator=g).to(dev)
    torch.manual_seed(0)
    nets = {"stock": RefineNet().to(dev), "hip": RefineNet().to(dev)}
    nets["hip"].load_state_dict(nets["stock"].state_dict())
    nets["stock"].hip_pass, nets["hip"].hip_pass = False, True
    for net in nets.values():                     # meaningful running statistics for the frozen / eval modes
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.momentum = 1.0
        net.train()
        with torch.no_grad():
            net(imgs[:, 0], depth)
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.momentum = 0.1
    nets["hip"].load_state_dict(nets["stock"].state_dict())
    for mode in ("train", "frozen", "eval"):
        last = {}
        steps = []
        for tag, net in nets.items():
            set_mode(net, mode)
            assert (net.hip_pass_mode(imgs[:, 0], depth) is not None) == (tag == "hip")
            steps.append((tag, make_step(net, mode, imgs, depth, gout, last, tag)))
        times = {tag: [] for tag, _ in steps}
        for r in range(WARMUP + ROUNDS):
            for tag, fn in steps:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if r >= WARMUP:
                    times[tag].append(e0.elapsed_time(e1))
        row = {tag: summary(ms) for tag, ms in times.items()}
        row["out_rel_l1_hip_vs_stock"] = float((last["hip"] - last["stock"]).abs().mean() / last["stock"].abs().mean())
        row["hip_p90_below_stock_p10"] = bool(row["hip"]["p90_ms"] < row["stock"]["p10_ms"])
        row["ratio_stock_over_hip_median"] = row["stock"]["median_ms"] / row["hip"]["median_ms"]
        wins[mode] = wins[mode] and row["hip_p90_below_stock_p10"]
        res["cases"]["%dx%d %s" % (H, W, mode)] = row
        nets["hip"].load_state_dict(nets["stock"].state_dict())      # (train mode moved the running statistics: the same again)
res["default_on_modes"] = sorted(m for m, ok in wins.items() if ok)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(res, fh, indent=1)
    fh.write("\n")
print(json.dumps(res))
