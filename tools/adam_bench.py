#!/usr/bin/env python3
"""Timing evidence for the optimiser step on one GPU, at MVSNet's and CVP-MVSNet's real parameter sets, three variants alternated
inside one process:
  (a) what bench.py does: bucket.gather() + torch.optim.Adam(bucket.optimizer_params(32), fused=True).step();
  (b) optim.FlatAdam.step() on the table path (the kernel reads the .grad tensors in place);
  (c) optim.FlatAdam.step() on the flat path (bucket.gather() + the flat kernel: the path behind a collective / under capture).
Every repetition of every variant gets FRESH .grad tensors, allocated and filled outside the timed region, laid out with the
parameters' strides as autograd leaves them.  Per variant: device time from one torch.cuda.Event pair per repetition (median, 10th /
90th percentile over 60 repetitions after 10 warm-up rounds), launch-thread time per call (host clock around the enqueue, no
synchronise inside), and the launches of one call (their names from the torch profiler; the library's own from its launch trace).
Writes one JSON object to profiles/adam_timing.json (or --out) and prints it."""
import argparse
import copy
import json
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import mvs_amd  # noqa: F401
from mvs_amd import _lib
from mvs_amd.dist import FlatGradBucket
from mvs_amd.optim import FlatAdam

REPS, WARMUP = 60, 10
dev = torch.device("cuda:0")


def models():
    from mvs_amd.jdacs.models.mvsnet import MVSNet
    from mvs_amd.jdacs_ms.models.network import CVPMVSNet
    torch.manual_seed(0)
    yield "MVSNet", MVSNet(refine=False)
    yield "CVP-MVSNet", CVPMVSNet(SimpleNamespace(nsrc=2, nscale=3, mode="test"))


def profiled_launches(prepare, fn):
    """names of the device kernels / copies / memsets ONE call of fn enqueues, from the torch profiler (None where it is unavailable);
    prepare() runs outside the profiled region"""
    try:
        from torch.profiler import ProfilerActivity, profile
        prepare()
        fn()
        prepare()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        return [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]       # a user annotation's device-side span included
    except Exception as exc:  # noqa: BLE001
        sys.stderr.write("launch count unavailable: %r\n" % (exc,))
        return None


def quantiles(xs):
    xs = sorted(xs)
    q = lambda f: xs[min(len(xs) - 1, int(f * len(xs)))]
    return {"median": q(0.5), "p10": q(0.1), "p90": q(0.9)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_timing.json"))
    args = ap.parse_args()
    lib = _lib.get()
    res = {"what": "optimiser step: (a) bucket.gather() + torch.optim.Adam(optimizer_params(32), fused=True), (b) FlatAdam table path, "
                   "(c) FlatAdam flat path; fresh .grad tensors per repetition, variants alternated in one process",
           "device": torch.cuda.get_device_name(0), "reps": REPS, "warmup": WARMUP, "models": {}}
    for name, net in models():
        nets = {k: copy.deepcopy(net).to(dev) for k in "abc"}
        params = {k: [p for p in nets[k].parameters() if p.requires_grad] for k in "abc"}
        bucket_a = FlatGradBucket(nets["a"].parameters(), flatten_params=True)
        opt_a = torch.optim.Adam(bucket_a.optimizer_params(32), lr=1e-4, betas=(0.9, 0.999), fused=True)
        opt_b = FlatAdam(nets["b"].parameters(), lr=1e-4, betas=(0.9, 0.999))
        opt_c = FlatAdam(nets["c"].parameters(), lr=1e-4, betas=(0.9, 0.999))
        opt_c.force_flat = True

        def step_a():
            bucket_a.gather()
            opt_a.step()

        steps = {"a": step_a, "b": opt_b.step, "c": opt_c.step}
        gen = torch.Generator(device=dev).manual_seed(1)
        src = [torch.randn(p.shape, device=dev, generator=gen) * 1e-3 for p in params["a"]]

        def fresh(k):
            for p, g in zip(params[k], src):
                p.grad = torch.empty_strided(p.shape, p.stride(), dtype=p.dtype, device=dev).copy_(g)

        dev_ms, host_ms = {k: [] for k in "abc"}, {k: [] for k in "abc"}
        for rep in range(WARMUP + REPS):
            for k in "abc":
                fresh(k)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                t0 = time.perf_counter()
                steps[k]()
                t1 = time.perf_counter()
                e1.record()
                e1.synchronize()
                if rep >= WARMUP:
                    dev_ms[k].append(e0.elapsed_time(e1))
                    host_ms[k].append((t1 - t0) * 1e3)
        # after the same number of steps from the same start the three parameter sets agree to fp32 rounding
        flat = {k: torch.cat([p.detach().reshape(-1) for p in params[k]]) for k in "abc"}
        row = {"tensors": len(params["a"]), "elements": int(flat["a"].numel()),
               "max_abs_difference_b_vs_a": float((flat["b"] - flat["a"]).abs().max()),
               "b_and_c_bit_identical": bool(torch.equal(flat["b"].view(torch.int32), flat["c"].view(torch.int32)))}
        labels = {"a": "a_gather_plus_torch_fused_adam", "b": "b_flat_adam_table", "c": "c_flat_adam_flat"}
        for k in "abc":
            fresh(k)
            lib.launch_trace()
            steps[k]()
            trace = lib.launch_trace()
            fresh(k)
            row[labels[k]] = {"device_ms": quantiles(dev_ms[k]), "launch_thread_ms": quantiles(host_ms[k]), "library_launch_trace": trace,
                              "profiled_launch_names": profiled_launches(lambda: fresh(k), steps[k])}
            names = row[labels[k]]["profiled_launch_names"]
            # "Optimizer.step#<class>.step" is the device-side span of torch.optim's own profiler annotation, not a launch
            row[labels[k]]["profiled_launches"] = None if names is None else sum(1 for nm in names if not nm.startswith("Optimizer.step#"))
        a = row[labels["a"]]["device_ms"]
        for k in "bc":
            mine = row[labels[k]]["device_ms"]
            row["%s_p90_below_a_p10" % k] = bool(mine["p90"] < a["p10"])
            row["ratio_a_over_%s_median" % k] = a["median"] / mine["median"]
        res["models"][name] = row
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
