#!/usr/bin/env python3
"""Timing evidence for the JDACS co-segmentation loss at the training shape (B = 1, N = 7, K = 4, features [7,512,14,14] ->
V [1372,512], depth 128x160) on one GPU:
  (a) the NMF solve alone (ops.nmf_solve, 50 iterations);
  (b) the segmentation loss forward + backward alone (ops.seg_loss);
  (c) tests/seg_oracle.py's fp32 composition of the same two on the same GPU: the reference's op sequence on ROCm, with its
      host synchronisations (the stopping test every tenth iteration).
Each is timed with torch.cuda.Event pairs after warm-up, one pair per repetition; reported are the median, the 10th / 90th
percentiles and the spread p90 - p10.  Writes one JSON object to profiles/seg_loss_timing.json and prints it."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import mvs_amd  # noqa: F401
from mvs_amd import ops
import seg_oracle as S

REPS, WARMUP = 40, 8
dev = torch.device("cuda:0")
b, n, k, h, w, iters, tol = 1, 7, 4, 128, 160, 50, 1e-4
V = S.relu_like_matrix(n * 14 * 14, 512, k, 15)
W0, H0 = S.nmf_initial_factors(V, k, 1)
Vd, W0d, H0d = V.to(dev), W0.to(dev), H0.to(dev)
Wsol, _, status = ops.nmf_solve(Vd, W0d, H0d, max_iter=iters, tol=tol)
heat, cams, depth = S.conditioned_seg_inputs(Wsol.cpu().view(b, n, 14, 14, k), b, n, h, w, seed=70)
heat = heat.to(dev)
cams, depth = cams.to(dev), depth.to(dev).requires_grad_(True)
ref_seg, view_segs = S.maps_at_depth_resolution(heat, h, w)
ref_seg = ref_seg.contiguous()
views = [view_segs[:, v].contiguous() for v in range(n - 1)]
kinv, proj = ops.unsup_view_transforms(cams)


def solve():
    ops.nmf_solve(Vd, W0d, H0d, max_iter=iters, tol=tol)


def loss():
    depth.grad = None
    ops.seg_loss(depth, ref_seg, views, kinv, proj)[0].backward()


def reference_ops():
    depth.grad = None
    Wr = S.nmf_iterate(Vd, W0d, H0d, True, iters, tol)[0]
    S.seg_loss(Wr.view(b, n, 14, 14, k), cams, depth).backward()


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
    return {"median_ms": q(0.5), "p10_ms": q(0.1), "p90_ms": q(0.9), "spread_ms": q(0.9) - q(0.1), "reps": REPS}


def launches(fn):
    """device kernels + memsets one call enqueues, counted by the torch profiler (None where it is unavailable)"""
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


res = {"what": "JDACS co-segmentation loss, B=1 N=7 K=4, V [1372,512], depth 128x160, 50 NMF iterations (tol 1e-4)",
       "device": torch.cuda.get_device_name(0), "nmf_iterations_run": int(status[0, 0]),
       "a_nmf_solve": timed(solve), "b_seg_loss_fwd_bwd": timed(loss), "c_reference_ops": timed(reference_ops),
       "library_launches": {"a_nmf_solve": 2 * iters + 2, "b_seg_loss_fwd": 2, "b_seg_loss_bwd": 1},
       "profiled_launches": {"a_nmf_solve": launches(solve), "b_seg_loss_fwd_bwd": launches(loss), "c_reference_ops": launches(reference_ops)}}
ab = res["a_nmf_solve"]["median_ms"] + res["b_seg_loss_fwd_bwd"]["median_ms"]
res["a_plus_b_median_ms"] = ab
res["ratio_c_over_a_plus_b"] = res["c_reference_ops"]["median_ms"] / ab
res["a_plus_b_below_c_by_more_than_spread"] = bool(
    res["c_reference_ops"]["median_ms"] - ab > max(res["a_nmf_solve"]["spread_ms"] + res["b_seg_loss_fwd_bwd"]["spread_ms"],
                                                   res["c_reference_ops"]["spread_ms"]))
out = os.path.join(ROOT, "profiles", "seg_loss_timing.json")
with open(out, "w") as fh:
    json.dump(res, fh, indent=1)
    fh.write("\n")
print(json.dumps(res))
