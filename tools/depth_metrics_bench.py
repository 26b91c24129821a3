#!/usr/bin/env python3
"""Timing evidence for the seven depth-map validation metrics on one GPU, at B = 4, 128 x 160 (training resolution) and B = 1,
1200 x 1600 (eval_dense):
  (a) ops.depth_metrics: the launch pair of csrc/depth_metrics_kernels.h, nothing read back;
  (b) tests/metrics_oracle.py:train_block on the same GPU: the reference's op sequence for the same seven values with stock
      PyTorch-ROCm ops -- the Python loop over the batch with its boolean-mask selections, the repeat()-ed interval images, and
      one .item() per scalar as tensor2float does.
Each is timed with torch.cuda.Event pairs after 8 warm-up runs, one pair per repetition, 40 repetitions; reported are the median
and the 10th / 90th percentiles.  Also counted per call: kernel launches ((a) from the library's launch trace, both from the torch
profiler) and host synchronisations (torch's sync-debug mode "warn": one warning per synchronising call).
Writes one JSON object to profiles/depth_metrics_timing.json and prints it."""
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import mvs_amd  # noqa: F401
from mvs_amd import _lib, ops
import metrics_oracle as M

REPS, WARMUP = 40, 8
SHAPES = {"train_B4_128x160": (4, 128, 160, 171), "eval_dense_B1_1200x1600": (1, 1200, 1600, 172)}
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
    return {"median_ms": q(0.5), "p10_ms": q(0.1), "p90_ms": q(0.9), "spread_ms": q(0.9) - q(0.1), "reps": REPS, "warmup": WARMUP}


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
    """synchronising calls of one run of fn, as torch's sync-debug mode reports them (its own one-time notice that the mode is a
    prototype is not one)"""
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


lib = _lib.get()
res = {"what": "seven depth-map validation metrics (jdacs/train.py:232-238): (a) ops.depth_metrics, (b) the reference's op sequence "
               "with stock PyTorch-ROCm ops incl. one .item() per scalar",
       "device": torch.cuda.get_device_name(0), "shapes": {}}
for name, (b, h, w, seed) in SHAPES.items():
    est, gt, mask, interval = M.seeded_inputs(b, h, w, seed, device=dev)

    def ours():
        return ops.depth_metrics(est, gt, mask, interval, M.THRESHOLDS)

    def reference_ops():
        return M.train_block(est, gt, mask, interval)

    out = ours()[0]
    vals = reference_ops()[0]
    worst = max(abs(float(out[i]) - vals[k]) / abs(vals[k]) for i, k in enumerate(M.KEYS))
    lib.launch_trace()
    ours()
    trace = lib.launch_trace()
    row = {"B": b, "H": h, "W": w, "a_depth_metrics": timed(ours), "b_reference_ops": timed(reference_ops),
           "a_library_launches": len(trace), "a_launch_trace": trace,
           "profiled_launches": {"a_depth_metrics": profiled_launches(ours), "b_reference_ops": profiled_launches(reference_ops)},
           "host_syncs": {"a_depth_metrics": host_syncs(ours), "b_reference_ops": host_syncs(reference_ops),
                          "b_counted_from_the_op_sequence": M.host_syncs_of_train_block(b)},
           "max_relative_difference_a_vs_b": worst}
    row["ratio_b_over_a_median"] = row["b_reference_ops"]["median_ms"] / row["a_depth_metrics"]["median_ms"]
    row["a_p90_below_b_p10"] = bool(row["a_depth_metrics"]["p90_ms"] < row["b_reference_ops"]["p10_ms"])
    res["shapes"][name] = row
out_dir = os.path.join(ROOT, "profiles")
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "depth_metrics_timing.json"), "w") as fh:
    json.dump(res, fh, indent=1)
    fh.write("\n")
print(json.dumps(res))
