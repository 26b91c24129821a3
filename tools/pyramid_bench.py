#!/usr/bin/env python3
"""Timing evidence for FeaturePyramid.hip_pass on one GPU: forward + backward of the CVP feature pyramid alone
(jdacs-ms/models/network.py:16-50) through the one-node HIP pass (ops.FeaturePyramidFn) against the per-layer path it replaces
(hip_pass = False: F.interpolate + a layout copy per level, nine ops.Conv2dLReLUFn nodes per level), on the same weights, the same
images and the same fixed upstream gradients for every level.
  shapes (N, H, W, S): (28, 128, 160, 2) -- jdacs-ms/train.sh per GPU at 8 GPUs: 4 samples x 7 views, nscale 2 --, (56, 128, 160, 2)
                       -- the same recipe at 4 GPUs --, (7, 128, 160, 2) -- one sample
A step is zero_grad + forward + backward.  The two variants are INTERLEAVED -- one step of each per round -- after 8 warm-up rounds,
40 rounds; reported per variant are the median and the 10th / 90th percentiles of the time between torch.cuda.Event pairs and of the
launch thread's time (host clock from the start of the step until backward() returns, no synchronise inside), and the number of
device kernels / memcpy / memset activities of one step from torch.profiler (a run of its own after the timing).
The rule of DESIGN.md section 7 decides the default: on only if the node's p90 is below the per-layer path's p10 at the recipe shape.
Writes one JSON object to profiles/pyramid_timing.json (--out) and prints it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import mvs_amd  # noqa: F401
from mvs_amd.jdacs_ms.models.network import FeaturePyramid

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyramid_timing.json"))
ap.add_argument("--rounds", type=int, default=40)
ap.add_argument("--warmup", type=int, default=8)
args = ap.parse_args()
ROUNDS, WARMUP = args.rounds, args.warmup
SHAPES = ((28, 128, 160, 2), (56, 128, 160, 2), (7, 128, 160, 2))
RECIPE = SHAPES[0]
assert torch.cuda.is_available(), "pyramid_bench measures on the GPU"
dev = torch.device("cuda:0")


def summary(vals):
    vals = sorted(vals)
    q = lambda f: vals[min(len(vals) - 1, int(f * len(vals)))]
    return {"median_ms": q(0.5), "p10_ms": q(0.1), "p90_ms": q(0.9)}


def make_step(net, img, S, gouts, last, tag):
    def run():
        net.zero_grad(set_to_none=True)
        outs = net(img, S)
        torch.autograd.backward(outs, gouts)
        last[tag] = outs
    return run


def device_activities(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]
    copies = sum(n.startswith(("Memcpy", "Memset")) for n in names)
    ours = sum(n.startswith(("conv2d_", "pyramid_", "void conv2d_", "void pyramid_")) for n in names)
    return {"device_activities": len(names), "library_kernels": ours, "memcpy_memset": copies, "other_kernels": len(names) - ours - copies}


res = {"what": "FeaturePyramid alone, zero_grad + forward + backward with fixed upstream gradients for every level: per_layer = "
               "hip_pass False (nine Conv2dLReLUFn nodes per level, the parent commit's behaviour), node = ops.FeaturePyramidFn; interleaved rounds",
       "device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "warmup": WARMUP, "cases": {}}
for N, H, W, S in SHAPES:
    g = torch.Generator().manual_seed(N + H + W)
    img = torch.randn(N, 3, H, W, generator=g).to(dev)
    gouts = [torch.randn(N, 16, H >> s, W >> s, generator=g).to(dev).contiguous(memory_format=torch.channels_last) for s in range(S)]
    torch.manual_seed(0)
    nets = {"per_layer": FeaturePyramid().to(dev), "node": FeaturePyramid().to(dev)}
    nets["node"].load_state_dict(nets["per_layer"].state_dict())
    nets["per_layer"].hip_pass, nets["node"].hip_pass = False, True
    last, steps = {}, []
    for tag, net in nets.items():
        net.train()
        assert (net.hip_pass_slope(img) is not None) == (tag == "node")
        steps.append((tag, make_step(net, img, S, gouts, last, tag)))
    ev, host = {tag: [] for tag, _ in steps}, {tag: [] for tag, _ in steps}
    for r in range(WARMUP + ROUNDS):
        for tag, fn in steps:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            t1 = time.perf_counter()
            e1.record()
            e1.synchronize()
            if r >= WARMUP:
                ev[tag].append(e0.elapsed_time(e1))
                host[tag].append((t1 - t0) * 1e3)
    row = {}
    for tag, fn in steps:
        row[tag] = {"events": summary(ev[tag]), "launch_thread": summary(host[tag])}
        row[tag].update(device_activities(fn))
    gn = {k: p.grad for k, p in nets["node"].named_parameters()}
    gp = {k: p.grad for k, p in nets["per_layer"].named_parameters()}
    row["features_equal_bits"] = [bool(torch.equal(a, b)) for a, b in zip(last["node"], last["per_layer"])]
    row["grad_rel_l1_node_vs_per_layer_max"] = max(float((gn[k] - gp[k]).abs().sum() / gp[k].abs().sum()) for k in gn)
    row["node_p90_below_per_layer_p10"] = bool(row["node"]["events"]["p90_ms"] < row["per_layer"]["events"]["p10_ms"])
    row["ratio_per_layer_over_node_median"] = row["per_layer"]["events"]["median_ms"] / row["node"]["events"]["median_ms"]
    res["cases"]["%dx%dx%dx%d" % (N, H, W, S)] = row
res["recipe_shape"] = "%dx%dx%dx%d" % RECIPE
res["default_on"] = bool(res["cases"][res["recipe_shape"]]["node_p90_below_per_layer_p10"])
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(res, fh, indent=1)
    fh.write("\n")
print(json.dumps(res))
