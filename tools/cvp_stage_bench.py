#!/usr/bin/env python3
"""Timing evidence for CVPMVSNet.hip_stage on one GPU: the whole CVPMVSNet forward with the stage glue off (the ATen launches and the
solver library's LU inverses between this library's kernels) and on (ops.cvp_cameras + ops.depth_hypotheses_up), alternated inside one
process on the same model and inputs, at two shapes:

  recipe    the jdacs-ms training recipe per GPU: B = 4, nsrc = 6, 128x160, nscale = 2, train mode, autograd on
  config4   BASELINE configs[3]: B = 1, nsrc = 4, 864x1152, nscale = 3, eval mode under no_grad

Per shape and variant: device time from one torch.cuda.Event pair per forward and launch-thread time (host clock around the forward,
no synchronise inside), each as median with 10th / 90th percentile over --reps forwards after --warmup rounds; the device activities of
one forward from torch.profiler (a run of its own, after the timing), split into this library's kernels (names read from csrc/) and the
rest; the library's launch labels that differ.  `default_on_by_rule` is DESIGN.md section 7's rule: the stage's p90 below the old
path's p10, event time, at BOTH shapes.  Writes one JSON object to profiles/cvp_stage_timing.json (or --out) and prints it."""
import argparse
import json
import os
import re
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

import mvs_amd  # noqa: F401
from mvs_amd import _lib, synthetic
from mvs_amd.jdacs_ms.models.network import CVPMVSNet

SHAPES = {"recipe": dict(B=4, nsrc=6, H=128, W=160, nscale=2, train=True),
          "config4": dict(B=1, nsrc=4, H=864, W=1152, nscale=3, train=False)}
VARIANTS = (("stage_off", False), ("stage_on", True))


def kernel_names():
    names = set()
    csrc = os.path.join(ROOT, "self-supervised-mvs_amd", "csrc")
    for fn in os.listdir(csrc):
        if fn.endswith((".hip", ".h", ".cpp")):
            names.update(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", open(os.path.join(csrc, fn)).read()))
    return names


def quantiles(xs):
    xs = sorted(xs)
    q = lambda f: xs[min(len(xs) - 1, int(f * len(xs)))]
    return {"median": q(0.5), "p10": q(0.1), "p90": q(0.9)}


def inputs(dev, B, nsrc, H, W):
    gen = torch.Generator().manual_seed(4)
    K, E = synthetic.synthetic_cameras(nsrc + 1, H, W, W)
    smooth = lambda n: F.avg_pool2d(torch.randn(n, 3, H, W, generator=gen), 5, 1, 2)
    ins = [smooth(B), smooth(B * nsrc).view(B, nsrc, 3, H, W), K.unsqueeze(0).repeat(B, 1, 1), K.view(1, 1, 3, 3).repeat(B, nsrc, 1, 1),
           E[0].unsqueeze(0).repeat(B, 1, 1), E[1:].unsqueeze(0).repeat(B, 1, 1, 1), torch.full((B,), 425.0), torch.full((B,), 425.0 + 47 * 13.5)]
    return [t.to(dev) for t in ins]


def run_shape(lib, dev, cfg, reps, warmup, ours):
    torch.manual_seed(0)
    net = CVPMVSNet(SimpleNamespace(nsrc=cfg["nsrc"], nscale=cfg["nscale"], mode="train" if cfg["train"] else "test")).to(dev)
    net.train(cfg["train"])
    ins = inputs(dev, cfg["B"], cfg["nsrc"], cfg["H"], cfg["W"])

    def forward(stage):
        net.hip_stage = stage
        with torch.set_grad_enabled(cfg["train"]):
            return net(*ins)

    dev_ms, host_ms = {k: [] for k, _ in VARIANTS}, {k: [] for k, _ in VARIANTS}
    for rep in range(warmup + reps):
        for name, stage in VARIANTS:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            out = forward(stage)
            t1 = time.perf_counter()
            e1.record()
            e1.synchronize()
            del out
            if rep >= warmup:
                dev_ms[name].append(e0.elapsed_time(e1))
                host_ms[name].append((t1 - t0) * 1e3)
    row = {"shape": cfg, "reps": reps, "warmup": warmup}
    outs = {}
    from torch.profiler import ProfilerActivity, profile
    for name, stage in VARIANTS:
        lib.launch_trace()
        outs[name] = [d.detach() for d in forward(stage)["depth_est_list"]]
        labels = lib.launch_trace()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            forward(stage)
            torch.cuda.synchronize()
        acts = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]
        foreign = [n for n in acts if not any(t in ours for t in re.findall(r"\w+", n))]
        counts = {}
        for n in foreign:
            counts[n] = counts.get(n, 0) + 1
        row[name] = {"event_ms": quantiles(dev_ms[name]), "launch_thread_ms": quantiles(host_ms[name]),
                     "device_activities": len(acts), "library_kernels": len(acts) - len(foreign), "other_activities": len(foreign),
                     "other_activity_names": counts,
                     "stage_labels_in_first_64": [lab for lab in labels if lab in ("cvp_cameras", "depth_hypo_up_interval", "depth_hypo_up_write",
                                                                                  "relative_projection", "depth_hypo")]}
    off, on = row["stage_off"], row["stage_on"]
    row["on_p90_below_off_p10_event"] = bool(on["event_ms"]["p90"] < off["event_ms"]["p10"])
    row["on_p90_below_off_p10_launch_thread"] = bool(on["launch_thread_ms"]["p90"] < off["launch_thread_ms"]["p10"])
    row["event_ms_saved_median"] = off["event_ms"]["median"] - on["event_ms"]["median"]
    row["launch_thread_ms_saved_median"] = off["launch_thread_ms"]["median"] - on["launch_thread_ms"]["median"]
    # the same geometry with differently rounded camera products: relative L1 distance of every level's depth map, finest first
    row["depth_rel_l1_on_vs_off"] = [float((a - b).abs().mean() / b.abs().mean()) for a, b in zip(outs["stage_on"], outs["stage_off"])]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cvp_stage_timing.json"))
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="recipe,config4")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cvp_stage_bench: needs the GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    lib = _lib.get()
    ours = kernel_names()
    res = {"what": "CVPMVSNet forward, stage glue off / on (CVPMVSNet.hip_stage), alternated in one process; ms",
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in args.shapes.split(","):
        res["shapes"][name] = run_shape(lib, dev, SHAPES[name], args.reps, args.warmup, ours)
        sys.stderr.write("%s done\n" % name)
    res["default_on_by_rule"] = bool(res["shapes"]) and set(res["shapes"]) == set(SHAPES) and \
        all(r["on_p90_below_off_p10_event"] for r in res["shapes"].values())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
