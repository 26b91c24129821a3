#!/usr/bin/env python3
"""bench.py -- depth-samples/s of the MVSNet hot path on MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

One step = one pass of the hot path over one batch of synthetic DTU-shaped input on every rank:
BASELINE config 2 -- MVSNet (refine off), N=3 views, 640x512 images, D=192, fp32, forward + loss
(mvsnet_loss, jdacs/models/mvsnet.py:164) + backward + gradient all-reduce (RCCL, N>1) + Adam step, every step from the same
parameters and optimiser state (restored in front of it: one copy, one memset).
1 sample per GPU per step (weak scaling, like the reference's batch 1/GPU recipe, jdacs/train.sh).
Inputs are resident in HBM before the timed region.  Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times the K
steps and prints the line; --full adds the per-kernel / roofline figures, the other modes' timings and the CPU / stock-PyTorch
baselines; --dump-outputs DIR writes what the last timed step computed as DIR/<name>.npy.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_ROCTX = None
if os.environ.get("MVS_ROCTX"):
    # rocprofv3 --selected-regions: rocprofiler-sdk's roctx library has to be in the process before torch brings its own
    # (older, without roctxProfilerPause / Resume) libroctx64 and before the HIP runtime starts
    import ctypes
    for _name in ("/opt/rocm/lib/librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so"):
        try:
            _cand = ctypes.CDLL(_name, mode=ctypes.RTLD_GLOBAL)
            _cand.roctxProfilerPause.argtypes = [ctypes.c_uint64]
            _cand.roctxProfilerResume.argtypes = [ctypes.c_uint64]
            _ROCTX = _cand
            break
        except (OSError, AttributeError):
            continue
    if _ROCTX is None:
        sys.stderr.write("MVS_ROCTX: no roctx library with roctxProfilerPause / Resume; the whole run is profiled\n")

import torch
import torch.distributed as dist

# BASELINE.json configs (index = --config): [1] is the headline (`metric` is quoted on it) and the default
HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
MFMA_F32_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: fp32-input MFMA == fp32 vector peak
FEAT_C = 32
CONFIGS = {
    2: dict(views=3, image=(512, 640), planes=192, kind="train",
            what="MVSNet N=3 640x512 D=192 fp32 forward+loss+backward+allreduce+Adam, 1 sample/GPU/step (BASELINE configs[1])"),
    3: dict(views=5, image=(512, 640), planes=192, kind="selfsup",
            what="JDACS self-supervised step: MVSNet N=5 640x512 D=192 fp32 forward + UnSupLoss (photometric+SSIM+smoothness) + "
                 "backward + allreduce + Adam, 1 sample/GPU/step (BASELINE configs[2]: batch 8 over 8 GPUs)"),
    4: dict(views=5, image=(864, 1152), planes=(48, 8, 8), kind="cvp_infer",
            what="JDACS-MS / CVP-MVSNet 3-level pyramid inference, final 1152x864, D=(48,8,8), N=5, fp32 (BASELINE configs[3]; "
                 "the reference runs this size in jdacs-ms/test.py only)"),
    5: dict(views=7, image=(1184, 1600), planes=256, kind="infer",
            what="MVSNet N=7 1600x1184 D=256 inference, cost volume resident in HBM (BASELINE configs[4])"),
}
NVIEWS, (IMG_H, IMG_W), NDEPTH = CONFIGS[2]["views"], CONFIGS[2]["image"], CONFIGS[2]["planes"]


def algorithmic_work(cfg):
    """Per-launch algorithmic bytes / flops of the tagged kernels (stated in DESIGN.md) and their call tags."""
    c = CONFIGS[cfg]
    if c["kind"] == "cvp_infer":
        # CVP-MVSNet finest level (D = 8 per-pixel hypotheses at the full 864x1152, 16 feature channels): the refine sweep (HBM:
        # features in, per-pixel hypotheses in, variance out) and the two layers that dominate the step (MFMA)
        n, (ih, iw) = c["views"], c["image"]
        d = c["planes"][-1]
        vox = d * ih * iw
        work = {"sweep_fwd": ("hbm", n * 16 * ih * iw * 4 + 16 * vox * 4 + vox * 4),
                "conv_64_64": ("mfma", 2 * 27 * 64 * 64 * (d // 2) * (ih // 2) * (iw // 2)),
                "conv_16_16": ("mfma", 2 * 27 * 16 * 16 * vox)}
        tags = {"sweep_fwd": ("mvs_plane_sweep_variance_fwd", "sweep_fwd:N%d:C16:1x%dx%dx%d" % (n, d, ih, iw)),
                "conv_64_64": ("mvs_conv3d_fwd", "fwd:64>64:s1:1x%dx%dx%d" % (d // 2, ih // 2, iw // 2)),
                "conv_16_16": ("mvs_conv3d_fwd", "fwd:16>16:s1:1x%dx%dx%d" % (d, ih, iw))}
        return work, tags
    n, (ih, iw), nd = c["views"], c["image"], c["planes"]
    hf, wf = ih // 4, iw // 4
    vox = nd * hf * wf
    dims = "1x%dx%dx%d" % (nd, hf, wf)
    work = {
        "sweep_fwd": ("hbm", n * FEAT_C * hf * wf * 4 + FEAT_C * vox * 4),            # config 2: 511 180 800 B
        "conv0_fwd": ("mfma", 2 * 27 * 32 * 8 * vox),                                 # config 2: 54.4 GFLOP
    }
    tags = {
        "sweep_fwd": ("mvs_plane_sweep_variance_fwd", "sweep_fwd:N%d:C32:%s" % (n, dims)),
        "conv0_fwd": ("mvs_conv3d_fwd", "fwd:32>8:s1:%s" % dims),
    }
    if cfg == 5:
        # bf16 storage: the sweep writes C*vox*2 bytes; conv0 at bf16 MFMA rates is HBM bound (reads 32, writes 8 channels in bf16)
        work.update({"sweep_fwd_bf16": ("hbm", n * FEAT_C * hf * wf * 4 + FEAT_C * vox * 2), "conv0_fwd_bf16": ("hbm", (FEAT_C + 8) * vox * 2)})
        tags.update({"sweep_fwd_bf16": ("mvs_plane_sweep_variance_fwd_bf16", "sweep_fwd_bf16:N%d:C32:%s" % (n, dims)),
                     "conv0_fwd_bf16": ("mvs_conv3d_bf16_fwd", "fwd_bf16:32>8:s1:%s" % dims)})
    if c["kind"] in ("train", "selfsup"):
        work.update({"sweep_bwd": ("hbm", FEAT_C * vox * 4 + 2 * n * FEAT_C * hf * wf * 4),   # config 2: 519 045 120 B
                     "conv0_wgrad": ("mfma", 2 * 27 * 32 * 8 * vox), "conv0_dgrad": ("mfma", 2 * 27 * 32 * 8 * vox)})
        tags.update({"sweep_bwd": ("mvs_plane_sweep_variance_bwd", "sweep_bwd:N%d:C32:%s" % (n, dims)),
                     "conv0_wgrad": ("mvs_conv3d_wgrad", "wgrad:32>8:s1:%s" % dims),
                     "conv0_dgrad": ("mvs_conv3d_dgrad", "dgrad:32>8:s1:%s" % dims)})
    return work, tags


# the kernel the roofline object describes (the longest-running tagged kernel of the step, profiles/r04_final_bench*.json): the ONLY
# one bracketed by HIP events inside the timed region -- every bracket is two event records on the launch stream (~5 us of stream
# time each; five bracketed kernels cost the headline ~0.1 ms/step in round 4's first sessions).  The other tagged kernels are timed
# in a second pass of the same K steps right after the region (--region-timers all: everything inside the region, as before).
DOMINANT = {2: "conv0_wgrad", 3: "sweep_bwd", 4: "conv_64_64", 5: "sweep_fwd_bf16"}

HIP_KERNEL_OF = {   # bench tag -> substring of the HIP kernel's name in the rocprofv3 output
    "sweep_fwd": "plane_sweep_variance_fwd", "sweep_bwd": "plane_sweep_variance_bwd",
    "conv0_fwd": "conv_c8_fwd_bc_kernel", "conv0_wgrad": "conv_c8_wgrad_gs_kernel", "conv0_dgrad": "conv_pers_kernel<0, 8, 2,",
    "sweep_fwd_bf16": "plane_sweep_variance_fwd", "conv0_fwd_bf16": "conv_bf16_kernel<",
    "conv_64_64": "conv_igemm_kernel<0, 16, 4", "conv_16_16": "conv_pers_kernel<0, 16, 1,",
}
# the tags tools/pmc_driver.py replays per --config (one kernel name per tag within a config: the substrings above are matched
# against that config's driver run only)
PMC_TAGS = {2: ("sweep_fwd", "sweep_bwd", "conv0_fwd", "conv0_wgrad", "conv0_dgrad"),
            3: ("sweep_fwd", "sweep_bwd", "conv0_fwd", "conv0_wgrad", "conv0_dgrad"),
            4: ("sweep_fwd", "conv_64_64", "conv_16_16"),
            5: ("sweep_fwd_bf16", "conv0_fwd_bf16", "sweep_fwd", "conv0_fwd")}


def pmc_traffic(cfg, dtype="f32"):
    """HBM traffic per launch of the roofline kernels: rocprofv3 PMC counters of tools/pmc_driver.py (the same kernels at
    the same shapes as --config), FETCH_SIZE and WRITE_SIZE in separate passes as MI355X_MICROARCH.md prescribes.  On gfx950
    FETCH_SIZE tallies every 128-byte line at 64 bytes (calibrated: tools/fetch_calib.hip, profiles/r01_run20_fetch_calib.log)
    -> doubled; WRITE_SIZE matched known byte counts as reported.  Both are in KiB."""
    import shutil
    import subprocess
    import tempfile
    if shutil.which("rocprofv3") is None:
        return None, "rocprofv3 not on PATH"
    root = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(root, "tools"))
    from pmc_summary import summarise
    tmp = tempfile.mkdtemp(prefix="mvs_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp", MVS_PMC_CONFIG=str(cfg), MVS_PMC_DTYPE=dtype)
    dirs = []
    # third pass: the SQ's instruction counters -- the plane-sweep kernels are bound by vector-ALU issue and latency, not by HBM
    # (DESIGN.md section 4), so their line carries an ISSUE-side ceiling next to the HBM fraction
    for counter in ("FETCH_SIZE", "WRITE_SIZE", "SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_BUSY_CYCLES"):
        d = os.path.join(tmp, counter.split()[0])
        r = subprocess.run(["rocprofv3", "--pmc"] + counter.split() + ["--kernel-trace", "--output-format", "csv", "-d", d, "-o", "pmc", "--",
                            sys.executable, os.path.join(root, "tools", "pmc_driver.py")],
                           cwd="/tmp", env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            shutil.rmtree(tmp, ignore_errors=True)
            err = r.stderr or r.stdout or ""
            at = err.rfind("Traceback")
            return None, "rocprofv3 --pmc %s failed: %s" % (counter, err[at:at + 1200] if at >= 0 else err[-600:])
        dirs.append(d)
    summ = summarise(dirs)
    shutil.rmtree(tmp, ignore_errors=True)
    out = {}
    for tag in PMC_TAGS.get(cfg, ()):
        if (dtype == "f32") == tag.endswith("_bf16") and cfg == 5:   # config 5 replays one storage dtype per run
            continue
        sub = HIP_KERNEL_OF[tag]
        for name, c in summ.items():
            if sub in name and "FETCH_SIZE" in c and "WRITE_SIZE" in c:
                out[tag] = {"fetch_bytes": 2.0 * 1024.0 * c["FETCH_SIZE"]["mean"], "write_bytes": 1024.0 * c["WRITE_SIZE"]["mean"],
                            "hip_kernel": name}
                if "SQ_INSTS_VALU" in c and "SQ_BUSY_CYCLES" in c:
                    # SQ_BUSY_CYCLES is summed over the 32 shader engines; a vector-ALU wave-instruction occupies its SIMD's issue port
                    # for 4 cycles (64 lanes on 16-lane hardware); 1024 SIMDs
                    cyc = c["SQ_BUSY_CYCLES"]["mean"] / 32.0
                    insts = c["SQ_INSTS_VALU"]["mean"]
                    out[tag]["sq"] = {"valu_wave_instructions": insts, "kernel_cycles": cyc,
                                      "valu_issue_cycles_per_simd": insts * 4.0 / 1024.0,
                                      "valu_issue_frac": insts * 4.0 / 1024.0 / cyc if cyc else None,
                                      "wave_cycles_quad": c.get("SQ_WAVE_CYCLES", {}).get("mean"),
                                      "waiting_frac_of_wave_time": (c["SQ_WAIT_ANY"]["mean"] / c["SQ_WAVE_CYCLES"]["mean"])
                                      if c.get("SQ_WAVE_CYCLES", {}).get("mean") and "SQ_WAIT_ANY" in c else None}
    note = ("rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes) of tools/pmc_driver.py at the --config %d shapes; "
            "FETCH_SIZE x2 (gfx950 counts 128-byte lines at 64 bytes)" % cfg)
    missing = [t for t in PMC_TAGS.get(cfg, ()) if t not in out and not ((dtype == "f32") == t.endswith("_bf16") and cfg == 5)]
    if missing:
        note += "; no counter rows matched %s among %s" % (missing, sorted(n[:60] for n in summ)[:12])
    return out, note


def wgrad_all_cus(lib, dev, dims, flops, groups_all=256, reps=12):
    """conv0's weight gradient with every CU (knob wgrad8_groups = 256), alone on the GPU, at the config's shape: the kernel's own
    quality next to the numbers of the launch the step uses (which is given FEWER workgroups on purpose: it runs on the side stream
    and the step is fastest when it leaves part of the chip to the main stream -- the A/B pairs are under profiles/)."""
    import ctypes
    from mvs_amd import _lib, ops as _o
    d, h, w = dims
    g = torch.Generator().manual_seed(7)
    cl = torch.channels_last_3d
    x = torch.randn(1, FEAT_C, d, h, w, generator=g).to(dev).contiguous(memory_format=cl)
    gy = torch.randn(1, 8, d, h, w, generator=g).to(dev).contiguous(memory_format=cl)
    cur = ctypes.c_int(0)
    lib.call("mvs_get_tuning", b"wgrad8_groups", ctypes.byref(cur))
    lib.call("mvs_set_tuning", b"wgrad8_groups", groups_all)
    try:
        with torch.no_grad():
            for _ in range(3):
                _o.conv3d_wgrad(x, gy, (8, FEAT_C, 3, 3, 3), 1, False)
            torch.cuda.synchronize()
            timer = _lib.KernelTimer(only={"mvs_conv3d_wgrad"}, names={"mvs_conv3d_wgrad"})
            prev, lib.profiler = lib.profiler, timer
            try:
                for _ in range(reps):
                    _o.conv3d_wgrad(x, gy, (8, FEAT_C, 3, 3, 3), 1, False)
                torch.cuda.synchronize()
            finally:
                lib.profiler = prev
    finally:
        lib.call("mvs_set_tuning", b"wgrad8_groups", int(cur.value))
    ms = sorted(a.elapsed_time(b) for evs in timer.events.values() for a, b in evs)
    if not ms:
        return {}
    print("[bench] conv0 weight gradient alone with %d workgroups, ms per call: %s" % (groups_all, " ".join("%.3f" % m for m in ms)), file=sys.stderr)
    ms = ms[len(ms) // 2]      # median of `reps` calls
    return {"ms_all_cus": ms, "frac_all_cus": flops / (ms * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS, "groups_in_step": int(cur.value),
            "all_cus_is": "the same kernel on the same shape with %d workgroups (one per CU) and nothing beside it, convolution + the "
                          "reduction of its partial images (the C-ABI call), on RANDOM operands right after the timed passes (median of "
                          "%d calls); in the step it is launched with `groups_in_step` workgroups on the side stream.  THIS is the "
                          "kernel's own quality as measured in this process; `frac` (in the step) is what the roofline object reports "
                          "(DESIGN.md section 4, 'reconciled': round 5's 77 %% was a best case and is withdrawn)" % (groups_all, reps)}


def host_cpu():
    """(model name, physical cores, logical CPUs) of this box from lscpu / os."""
    import subprocess
    model, cores, sockets = "unknown", None, 1
    try:
        for ln in subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout.splitlines():
            k, _, v = ln.partition(":")
            k, v = k.strip(), v.strip()
            if k == "Model name":
                model = v
            elif k == "Core(s) per socket":
                cores = int(v)
            elif k == "Socket(s)":
                sockets = int(v)
    except Exception:
        pass
    logical = os.cpu_count() or 1
    phys = cores * sockets if cores else logical
    try:
        phys = min(phys, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    return model, max(1, phys), logical


def cpu_baseline(net_state, seed):
    """The oracle (a torch-ops port of the reference path, pinned against the imported reference) timed on this box's host
    cores, SURVEY 8(d) protocol: torch threads = physical cores, 1 warm-up + 3 timed iterations, median.  Bounded sample of
    the benchmarked workload: ONE config-2 training sample (forward + loss + backward) per iteration; plus the config-1 line
    (eval forward N=3, 160x128, D=48: BASELINE configs[0], the reference's own CPU-runnable case)."""
    from oracle import ref_torch as R
    model, phys, logical = host_cpu()
    old_threads = torch.get_num_threads()
    torch.set_num_threads(phys)
    # the warp is timed as the reference's own F.grid_sample call (jdacs/models/module.py:136), not the oracle's hand-written
    # gather (1.96x slower on the CPU: VERDICT r2 #11); tests/test_oracle_golden.py asserts the two forms agree
    old_sampler = R.set_sampler("aten")
    try:
        oracle = R.OracleMVSNet(refine=False)
        oracle.load_state_dict(net_state)
        oracle.train()
        imgs, proj, dv = R.synthetic_mvsnet_inputs(1, NVIEWS, IMG_H, IMG_W, NDEPTH, seed=seed)
        gt = torch.full((1, IMG_H // 4, IMG_W // 4), 650.0)

        def sample():
            for p in oracle.parameters():
                p.grad = None
            t0 = time.perf_counter()
            out = oracle(imgs, proj, dv)
            R.mvsnet_loss(out["depth"], gt, torch.ones_like(gt)).backward()
            return time.perf_counter() - t0
        # Thread sweep FIRST (a stated baseline quotes its best configuration in `value`): threads = physical
        # cores oversubscribes this problem (128 threads: 10.8 s per sample, 16-32 threads: 4.4-4.8 s on the EPYC 9575F boxes), so one
        # warm-up + one timed sample per thread count, then 3 timed samples (median) at the fastest count -> `value`, `cores`.
        counts = sorted({t for t in (16, 32, 64) if t < phys} | {phys})
        sweep2 = {}
        for nt in counts:
            torch.set_num_threads(nt)
            sample()                               # warm-up (thread pool, allocator, oneDNN primitive cache)
            sweep2[nt] = round(sample(), 3)
            if sweep2[nt] > 40.0:
                break
        best2 = min(sweep2, key=sweep2.get)
        torch.set_num_threads(best2)
        sample()
        ts = sorted(sample() for _ in range(3))
        dt = ts[1]
        # config 1: eval forward at 160x128, D=48 (BASELINE configs[0]), the same protocol
        oracle.eval()
        i1, p1, d1 = R.synthetic_mvsnet_inputs(1, 3, 128, 160, 48, seed=seed)
        sweep1 = {}
        for nt in sorted({t for t in (8, 16, 32, 64) if t < phys} | {phys}):
            torch.set_num_threads(nt)
            with torch.no_grad():
                oracle(i1, p1, d1)
                tt = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    oracle(i1, p1, d1)
                    tt.append(time.perf_counter() - t0)
            sweep1[nt] = round(sorted(tt)[1], 4)
        best1 = min(sweep1, key=sweep1.get)
        c1 = sweep1[best1]
    finally:
        torch.set_num_threads(old_threads)
        R.set_sampler(old_sampler)
    return {"value": 1.0 / dt, "unit": "depth-samples/s", "cores": best2, "kind": "port", "cpu_model": model, "logical_cpus": logical,
            "physical_cores": phys, "seconds_per_sample": dt, "timed_runs_s": [round(t, 3) for t in ts],
            "sample": "the same workload (MVSNet N=3 640x512 D=192 fp32 fwd+loss+bwd, ONE sample per iteration) through oracle/ref_torch.py with "
                      "sampler='aten' (F.grid_sample called as the reference calls it, ATen/oneDNN conv3d, batch_norm, softmax): 1 warm-up + 1 timed "
                      "sample at each of %s torch threads, then 1 warm-up + 3 timed samples (median = value) at the fastest count, %d threads "
                      "(%d physical cores on the box)" % (sorted(sweep2), best2, phys),
            "seconds_per_sample_by_threads": {str(k): v for k, v in sorted(sweep2.items())},
            "config1": {"value": 1.0 / c1, "unit": "depth-samples/s", "seconds_per_sample": c1, "cores": best1,
                        "what": "BASELINE configs[0]: MVSNet eval forward N=3 160x128 D=48 on the same CPU, median of 3 after 1 warm-up at the "
                                "fastest thread count of the sweep",
                        "seconds_per_sample_by_threads": {str(k): v for k, v in sorted(sweep1.items())}}}


def calibrate_bn(net, *inputs):
    """Inference workloads: one train-mode pass with BatchNorm momentum 1, so the random-init model is evaluated with
    meaningful running statistics (with the defaults its logits are constant over depth: a degenerate workload)."""
    bns = [m for m in net.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    old = [m.momentum for m in bns]
    for m in bns:
        m.momentum = 1.0
    net.train()
    with torch.no_grad():
        net(*inputs)
    for m, mo in zip(bns, old):
        m.momentum = mo
    net.eval()


DUMP_MAX_ELEMS = 1 << 21    # per array (8 MB of float32, at most 8 arrays); a larger output is written as a fixed, seeded sample of its elements


def dump_outputs(folder, out, loss, bucket):
    """--dump-outputs: what a caller of the timed path received from its last step, as float32 .npy files -- the model's output
    dict and the loss; for the training configs also the all-reduced gradient bucket and the parameters the optimiser wrote."""
    import numpy as np
    arrays = {} if loss is None else {"loss": loss}
    for k, v in out.items():
        if isinstance(v, (list, tuple)):
            arrays.update(("%s_%d" % (k, i), t) for i, t in enumerate(v))
        else:
            arrays[k] = v
    if bucket is not None:
        arrays["grad_bucket"] = bucket.flat
        arrays["params"] = bucket.flat_param
    os.makedirs(folder, exist_ok=True)
    for name, t in arrays.items():
        a = t.detach().float().cpu().numpy()
        if a.size > DUMP_MAX_ELEMS:
            idx = np.sort(np.random.RandomState(0).choice(a.size, DUMP_MAX_ELEMS, replace=False))
            a = a.reshape(-1)[idx]
            name += "_sample"
        np.save(os.path.join(folder, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--region-timers", choices=("dominant", "all"), default="dominant",
                    help="HIP-event brackets inside the timed region: the roofline kernel only (default; the other tagged kernels in a "
                         "second pass of K steps after the region) or all tagged kernels")
    ap.add_argument("--step-events", type=int, default=0,
                    help="diagnostics: 1 = one HIP event after every timed step; the per-step GPU times go to the line as step_gpu_ms")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", type=int, default=2, choices=sorted(CONFIGS),
                    help="BASELINE.json configs index + 1: 2 (default, the headline metric's config) MVSNet N=3 train step; 3 JDACS "
                         "self-supervised step N=5; 4 CVP-MVSNet 3-level inference at 1152x864; 5 MVSNet N=7 1600x1184 D=256 inference")
    ap.add_argument("--dtype", type=str, default="", choices=["", "f32", "bf16"],
                    help="storage dtype of the cost volume / regulariser activations for --config 5 (default bf16 there; f32 elsewhere)")
    ap.add_argument("--batch", type=int, default=1,
                    help="samples per GPU per step of the training configs (default 1: the reference's recipe -- jdacs/train.sh: batch 4 over 4 "
                         "GPUs -- and what every round's headline was measured at); > 1: BatchNorm statistics over the rank's samples, "
                         "`value` counts samples, `config.samples_per_gpu_per_step` says so")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--gpu-reference", type=int, default=-1,
                    help="time the same step with the oracle's stock torch ops on this GPU (sampler='aten': F.grid_sample, MIOpen conv3d) = "
                         "'the reference GPU path' -> reference_gpu_path.  Default: on for the default N=1 config-2 run, off otherwise")
    ap.add_argument("--feature-channels-last", type=int, default=1,
                    help="1: run the stock-PyTorch FeatureNet in channels-last (MIOpen NHWC kernels)")
    ap.add_argument("--graph", type=int, default=0,
                    help="1: replay the whole step from a captured hipGraph (torch.cuda.CUDAGraph); 0: eager launches; "
                         "-1: try the graph, fall back to eager.  Default 0: the step is GPU-bound (profiles/), a replay buys nothing")
    ap.add_argument("--torch-profile", type=str, default="",
                    help="write a torch.profiler table (CPU + GPU, 5 steady-state steps) to this file (diagnostics)")
    ap.add_argument("--pmc", type=int, default=1,
                    help="1 (default, N=1 only): after the timed region run tools/pmc_driver.py under `rocprofv3 --pmc` (separate "
                         "FETCH_SIZE and WRITE_SIZE passes) to fill roofline.traffic; 0 or no rocprofv3 on PATH: traffic = null")
    ap.add_argument("--ab", type=str, default="",
                    help="interleaved A/B timing after the timed region (never the headline): ';'-separated toggles, each "
                         "'feature_fwd' (2-D extractor's forward through conv2d.hip + fused BatchNorm statistics) or "
                         "'<tuning key>=<value>' (mvs_set_tuning, against the library default); 5 pairs of --steps steps each")
    ap.add_argument("--ab-reps", type=int, default=5)
    ap.add_argument("--host-profile", type=str, default="",
                    help="after the timed region: cProfile of --steps more steps on the launch thread, top entries written to this file")
    ap.add_argument("--wgrad-streams", type=int, default=1,
                    help="side streams the regulariser's weight gradients are dealt to round-robin (ops.set_wgrad_streams)")
    ap.add_argument("--side-priority", type=str, default="default", choices=["default", "low", "high"],
                    help="priority of the weight-gradient side stream (ops.set_side_stream_priority)")
    ap.add_argument("--defer-join", type=int, default=0,
                    help="0 (default since round 6): the LIBRARY DEFAULT -- no set_async_wgrad opt-in; MVSNet's tail node "
                         "(ops.DeferredJoinFn) joins the regulariser's side-stream weight gradients at the end of the backward pass, safely "
                         "under gradient hooks; 1: round 5's opt-in (ops.set_async_wgrad(True, defer_join=True): the join by an autograd "
                         "engine callback, only for loops without gradient hooks)")
    ap.add_argument("--force-collective", action="store_true",
                    help="initialise the nccl (== RCCL) process group even at world size 1 and run the gradient bucket's all-reduce "
                         "inside every step: RCCL init + one ncclAllReduce of the flat bucket execute on a 1-GPU box")
    ap.add_argument("--sustained", type=int, default=0,
                    help="after everything else: this many MORE steps in the headline's mode with the garbage collector ON, reported "
                         "as ms_per_step_sustained (never the headline)")
    ap.add_argument("--dry-launch", action="store_true",
                    help="launcher check (tests, no GPU needed): start the ranks, all-reduce one number over gloo, print it, exit")
    ap.add_argument("--time-all-kernels", action="store_true",
                    help="extra untimed pass bracketing EVERY C-ABI call with HIP events (diagnostics to stderr)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: HIP-event brackets of the roofline kernel inside the timed region, the passes "
                         "after it (other tagged kernels, other weight-gradient modes, the opt-in split-bf16 step, the feature pyramid of "
                         "--config 4), PMC traffic, conv0's weight gradient on all CUs, cpu_baseline and reference_gpu_path.  Without it "
                         "the run sets up, warms up, times --steps steps, dumps its outputs if asked and prints the line")
    ap.add_argument("--dump-outputs", type=str, default="", metavar="DIR",
                    help="after the timed steps: write what the last timed step computed (depth, confidence, loss; for the training "
                         "configs also the all-reduced gradient bucket and the updated parameters) as DIR/<name>.npy in float32.  Every step "
                         "starts from the same state, so two runs agree to rounding (float atomics in the backward kernels)")
    args = ap.parse_args()
    full = args.full

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` on its own: start the N ranks here (one process per GPU, the reference starts all its
        # GPUs from one command too, jdacs/train.py:65) by re-executing under torch.distributed.run on the loopback address
        import socket
        import subprocess
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd, env=env))

    # exactly ONE line on stdout (the bench contract): libraries that talk on file descriptor 1 -- RCCL prints its version banner
    # there when a communicator is torn down -- are sent to stderr for the whole run; the JSON line goes to the saved descriptor
    sys.stdout.flush()
    _real_stdout = os.dup(1)
    os.dup2(2, 1)

    def emit(line):
        sys.stdout.flush()
        os.write(_real_stdout, (line + "\n").encode())

    import mvs_amd  # noqa: F401
    from mvs_amd import _lib, dist as mdist
    from mvs_amd.jdacs.models.mvsnet import MVSNet, mvsnet_loss
    from mvs_amd.synthetic import synthetic_mvsnet_inputs

    if args.dry_launch:
        rank, world, local = mdist.init_from_env("gloo")
        if world != args.gpus:
            raise SystemExit("bench.py: --gpus %d but the launcher started WORLD_SIZE=%d ranks" % (args.gpus, world))
        t = torch.tensor([float(rank + 1)])
        if world > 1:
            dist.all_reduce(t)
            dist.barrier()
        if rank == 0:
            emit(json.dumps({"dry_launch": True, "n_gpus": world, "rank_sum": float(t)}))
        if world > 1:
            dist.destroy_process_group()
        return
    t_pg = time.perf_counter()
    rank, world, local = mdist.init_from_env("nccl", force=args.force_collective)
    t_pg = time.perf_counter() - t_pg
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but the launcher started WORLD_SIZE=%d ranks" % (args.gpus, world))
    assert torch.cuda.is_available(), "bench.py needs MI355X GPUs"
    if local >= torch.cuda.device_count():
        raise SystemExit("bench.py: rank %d wants cuda:%d but only %d GPUs are visible" % (rank, local, torch.cuda.device_count()))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    # Self-diagnosis of the N > 1 path (no 8-GPU node has run this yet, so the first run that does must say what it
    # saw): the RCCL communicator is created lazily by the first collective -- time it, and COUNT the ranks with it (an all-reduce of
    # ones: the ncclCommCount equivalent), then gather which device every rank sits on.
    multi = None
    if dist.is_initialized():
        t_c = time.perf_counter()
        ones = torch.ones(1, dtype=torch.float32, device=dev)
        dist.all_reduce(ones)
        torch.cuda.synchronize()
        t_c = time.perf_counter() - t_c
        pr = torch.cuda.get_device_properties(dev)
        ident = torch.tensor([rank, local, getattr(pr, "pci_bus_id", -1) or -1, getattr(pr, "multi_processor_count", 0)], dtype=torch.int64, device=dev)
        idents = [torch.zeros_like(ident) for _ in range(dist.get_world_size())]
        dist.all_gather(idents, ident)
        multi = {"backend": dist.get_backend(), "process_group_init_s": round(t_pg, 3), "first_collective_s": round(t_c, 3),
                 "ranks_counted_by_all_reduce": int(round(float(ones.item()))), "world_size": dist.get_world_size(),
                 "rank_local_pcibus_cus": [[int(v) for v in t.tolist()] for t in idents],
                 "distinct_devices": len({(int(t[1]), int(t[2])) for t in idents})}
        if multi["ranks_counted_by_all_reduce"] != world:
            raise SystemExit("bench.py: the first all-reduce counted %d ranks, WORLD_SIZE is %d" % (multi["ranks_counted_by_all_reduce"], world))
    torch.backends.cudnn.benchmark = True  # as the reference does (jdacs/train.py:35); FeatureNet uses MIOpen

    cfg = CONFIGS[args.config]
    nviews, (img_h, img_w), ndepth = cfg["views"], cfg["image"], cfg["planes"]
    dtype = args.dtype or ("bf16" if args.config == 5 else "f32")
    if dtype == "bf16" and args.config != 5:
        raise SystemExit("bench.py: bf16 storage is the inference path of --config 5")
    torch.manual_seed(0)
    train = cfg["kind"] in ("train", "selfsup")
    bucket = opt = None
    last = {} if args.dump_outputs else None   # --dump-outputs: the outputs of the latest step (None: nothing is kept)
    if cfg["kind"] == "cvp_infer":
        from types import SimpleNamespace
        from mvs_amd.jdacs_ms.models.network import CVPMVSNet
        from mvs_amd.synthetic import synthetic_cameras
        net = CVPMVSNet(SimpleNamespace(nsrc=nviews - 1, nscale=3, mode="test"))
        state0 = None
        net = net.to(dev)
        g = torch.Generator().manual_seed(1 + rank)
        K, E = synthetic_cameras(nviews, img_h, img_w, img_w)
        cvp_in = [torch.randn(1, 3, img_h, img_w, generator=g), torch.randn(1, nviews - 1, 3, img_h, img_w, generator=g),
                  K.unsqueeze(0), K.view(1, 1, 3, 3).repeat(1, nviews - 1, 1, 1), E[0].unsqueeze(0), E[1:].unsqueeze(0),
                  torch.tensor([425.0]), torch.tensor([425.0 + 47 * 13.5])]
        cvp_in = [t.to(dev) for t in cvp_in]
        calibrate_bn(net, *cvp_in)    # BatchNorm running statistics := batch statistics of the random-init model

        def fwd_bwd():
            with torch.no_grad():
                out = net(*cvp_in)
            if last is not None:
                last["out"] = out
            return out["depth_est_list"][0].mean()
    else:
        net = MVSNet(refine=False, channels_last_features=bool(args.feature_channels_last))
        with torch.no_grad():
            net.cost_regularization.prob.weight.mul_(50.0)
        state0 = {k: v.clone() for k, v in net.state_dict().items()}
        net = net.to(dev).train()
        mdist.broadcast_parameters(net)
        imgs, proj, dv = synthetic_mvsnet_inputs(1, nviews, img_h, img_w, ndepth, seed=1 + rank)
        if args.batch > 1:
            if cfg["kind"] != "train":
                raise SystemExit("bench.py: --batch > 1 is implemented for --config 2")
            more = [synthetic_mvsnet_inputs(1, nviews, img_h, img_w, ndepth, seed=1 + rank + 1000 * k) for k in range(1, args.batch)]
            imgs = torch.cat([imgs] + [m[0] for m in more])
            proj = torch.cat([proj] + [m[1] for m in more])
            dv = torch.cat([dv] + [m[2] for m in more])
        if cfg["kind"] == "selfsup":
            import torch.nn.functional as F
            from mvs_amd.jdacs.losses.unsup_loss import UnSupLoss
            from mvs_amd.synthetic import synthetic_cameras
            # smooth textured images: the photometric loss needs an image gradient to be a meaningful workload
            imgs = F.avg_pool2d(imgs.view(nviews, 3, img_h, img_w), 9, 1, 4).view(1, nviews, 3, img_h, img_w) * 4
            K, E = synthetic_cameras(nviews, img_h // 4, img_w // 4, img_w)
            cams = torch.zeros(1, nviews, 2, 4, 4)
            cams[:, :, 0] = E
            cams[:, :, 1, :3, :3] = K
            cams = cams.to(dev)
            unsup = UnSupLoss()
        imgs, proj, dv = imgs.to(dev), proj.to(dev), dv.to(dev)
        gt = torch.full((max(1, args.batch), img_h // 4, img_w // 4), 650.0, device=dev)
        mask = torch.ones_like(gt)
        if train:
            # gradients AND parameters live in two flat fp32 buffers: one collective, one fused Adam launch
            bucket = mdist.FlatGradBucket(net.parameters(), flatten_params=True)
            bucket.force_collective = bool(args.force_collective)
            # capturable: the step counter lives on the GPU, so a captured optimizer step stays correct when replayed
            # (as 32 slices of the flat store: a fused multi-tensor optimiser runs one workgroup per tensor chunk)
            opt = torch.optim.Adam(bucket.optimizer_params(32), lr=1e-4, betas=(0.9, 0.999), fused=True, capturable=args.graph != 0)
            # Every step starts from the same parameters and optimiser state, so a step's results are a function of the inputs
            # alone.  Stepping on from the previous step's state instead, the last-bit differences of the float atomics in the
            # backward kernels grow from step to step (the peaky softmax + Adam): two identical 25-step runs ended 470 mm apart
            # in depth.  The optimiser state (exp_avg | exp_avg_sq | step of every slice) lives in ONE buffer, so the restore in
            # front of each step is two launches: a 1.35 MB copy and a memset.
            params0 = bucket.flat_param.detach().clone()
            slices = opt.param_groups[0]["params"]
            n_all = params0.numel()
            opt_state = torch.zeros(2 * n_all + len(slices), dtype=torch.float32, device=dev)
            off = 0
            for i, p in enumerate(slices):
                n = p.numel()
                opt.state[p] = {"step": opt_state[2 * n_all + i], "exp_avg": opt_state[off:off + n].view_as(p),
                                "exp_avg_sq": opt_state[n_all + off:n_all + off + n].view_as(p)}
                off += n

            def restore_state():
                with torch.no_grad():
                    bucket.flat_param.copy_(params0)
                opt_state.zero_()

            phase_marks = [] if args.step_events else None     # diagnostics: host clock after forward+loss / backward, per step

            def fwd_bwd():
                bucket.zero()
                out = net(imgs, proj, dv)
                if cfg["kind"] == "selfsup":
                    loss = unsup(imgs, cams, out["depth"])          # jdacs/train.py:199-210 (standard unsupervised loss)
                else:
                    loss = mvsnet_loss(out["depth"], gt, mask)
                if last is not None:
                    last["out"] = out
                if phase_marks is not None:
                    phase_marks.append(time.perf_counter())
                loss.backward()
                if phase_marks is not None:
                    phase_marks.append(time.perf_counter())
                bucket.gather()
                return loss
        else:
            calibrate_bn(net, imgs, proj, dv)   # BatchNorm running statistics := batch statistics of the random-init model
            if dtype == "bf16":
                net.storage_dtype = torch.bfloat16   # cost volume + regulariser activations stored in bf16, fp32 accumulation

            def fwd_bwd():
                with torch.no_grad():
                    out = net(imgs, proj, dv)
                if last is not None:
                    last["out"] = out
                return out["depth"].mean()

    def step():
        if train:
            restore_state()
        loss = fwd_bwd()
        if train:
            bucket.all_reduce()   # one RCCL all-reduce of the flat 1.35 MB bucket (no-op at world size 1)
            opt.step()
        return loss

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    lib = _lib.get()
    # weight gradients on a side HIP stream.  Since round 3 this is the LIBRARY default for the regulariser (ops.UNetRegulariserFn:
    # one autograd node, the side stream joined before its gradients are returned, so gradient hooks cannot see unfinished ones);
    # MVS_ASYNC_WGRAD=0 times the synchronous mode, and the line reports the other mode's ms/step beside the headline either way
    from mvs_amd import ops as _ops
    async_wgrad = os.environ.get("MVS_ASYNC_WGRAD", "1") != "0"
    # Round 6: the headline runs the LIBRARY DEFAULT (--defer-join 0): what a drop-in caller under the reference's train.py gets.  The
    # late join that round 5 measured as an opt-in now happens in MVSNet's tail node (ops.DeferredJoinFn), safely under gradient hooks.
    defer_join = bool(args.defer_join) and async_wgrad
    _ops.set_async_wgrad(async_wgrad, defer_join=defer_join)
    _ops.set_wgrad_streams(args.wgrad_streams)
    _ops.set_side_stream_priority(args.side_priority)
    eager_step = step
    graph_mode = False
    if args.graph != 0:
        # The step is ~300 short launches (ours + MIOpen + ATen); replaying them from one captured hipGraph
        # removes the host launch path from the critical path.  Same kernels, same work, same streams' order.
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    eager_step()       # MIOpen find + allocator warm-up must happen before capture
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            # two graphs with the collective launched eagerly between them, so RCCL is never captured and
            # the same code path runs at every world size
            graph_a, graph_b = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph_a):
                static_loss = fwd_bwd()
            with torch.cuda.graph(graph_b, pool=graph_a.pool()):
                if train:
                    opt.step()

            def step():  # noqa: F811
                if train:
                    restore_state()
                graph_a.replay()
                if train:
                    bucket.all_reduce()
                graph_b.replay()
                return static_loss
            step()
            torch.cuda.synchronize()
            graph_mode = True
        except Exception as e:
            if args.graph == 1:
                raise
            sys.stderr.write("hipGraph capture failed (%r); running eager\n" % (e,))
            step = eager_step
            torch.cuda.synchronize()
    roctx = _ROCTX   # rocprofv3 --selected-regions: collect the timed region only (no MIOpen find noise)
    # the cyclic garbage collector is kept out of the timed steps (an autograd step allocates ~10^4 Python objects; a generation-2
    # collection landing inside a step stalls the launch thread for 5-10 ms -- profiles/r04_run11: one 11.7 ms step among 4.0 ms ones);
    # one collection here, automatic collection back on after the region.  Reference counting frees everything as usual.
    # BEFORE the warm-up steps, not between them and the timed region: a full collection takes the launch thread tens of
    # milliseconds, the GPU drains and idles meanwhile, and the first timed steps then run at ramping clocks on an empty queue
    # (profiles/r04_run16: 7.4 / 5.65 / 5.45 / 5.32 ms for the first four timed steps against 5.26 in steady state).
    import gc
    gc.collect()
    gc.disable()
    t_warm = time.perf_counter()
    for _ in range(args.warmup):
        step()
    t_warm = time.perf_counter() - t_warm
    # live HIP-event timing of the roofline kernels over the timed region, on the launch stream
    work, tagmap = algorithmic_work(args.config)
    dom_key = DOMINANT.get(args.config) if (args.region_timers == "dominant" and DOMINANT.get(args.config) in tagmap) else None
    in_region = {k: v for k, v in tagmap.items() if dom_key is None or k == dom_key}
    later = {k: v for k, v in tagmap.items() if k not in in_region}
    timer = _lib.KernelTimer(only={t for _, t in in_region.values()}, names={n for n, _ in in_region.values()})
    if not graph_mode and full:
        lib.profiler = timer   # live HIP-event brackets inside the timed region (eager mode, --full)
    host_trace = None
    if args.step_events >= 2:
        class HostTrace:       # diagnostics: host clock at every C-ABI call of the timed steps (no HIP events)
            names = None
            rows = []

            def wants(self, name, tag):
                self.rows.append((time.perf_counter(), name, tag))
                return False
        host_trace = lib.profiler = HostTrace()
    t_gap = time.perf_counter()
    barrier()
    t_gap = time.perf_counter() - t_gap
    _ms0 = torch.cuda.memory_stats(dev)        # hipMalloc / hipFree calls of the caching allocator inside the timed region (should be 0: each one stalls the launch thread for milliseconds)
    if roctx is not None:
        roctx.roctxProfilerResume(0)
    t0 = time.perf_counter()
    host_marks = [t0]
    step_events = []
    if args.step_events and train:
        del phase_marks[:]
        _ops.JOIN_TRACE = []
    if args.step_events:
        step_events.append(torch.cuda.Event(enable_timing=True))
        step_events[0].record()
    for _ in range(args.steps):
        loss = step()
        host_marks.append(time.perf_counter())
        if args.step_events:
            step_events.append(torch.cuda.Event(enable_timing=True))
            step_events[-1].record()
    t_host = host_marks[-1] - t0            # the host has ENQUEUED the K steps (eager mode: Python + ctypes + allocator time)
    host_steps = sorted((b - a) * 1e3 for a, b in zip(host_marks, host_marks[1:]))
    barrier()
    dt = time.perf_counter() - t0
    _ms1 = torch.cuda.memory_stats(dev)
    alloc_diag = {k: int(_ms1.get(k, 0) - _ms0.get(k, 0)) for k in ("num_device_alloc", "num_device_free", "num_alloc_retries")}
    alloc_diag["reserved_bytes_end"] = int(_ms1.get("reserved_bytes.all.current", 0))
    if roctx is not None:
        roctx.roctxProfilerPause(0)
    gc.enable()
    lib.profiler = None
    join_trace, _ops.JOIN_TRACE = _ops.JOIN_TRACE, None
    if last is not None and rank == 0:
        dump_outputs(args.dump_outputs, last["out"], loss if train else None, bucket)
    if graph_mode and full:
        # kernels inside a graph replay cannot be bracketed by events; time the very same launches with HIP
        # events in an eager pass of the same K steps directly after the timed region (same process, same data)
        lib.profiler = timer
        for _ in range(args.steps):
            eager_step()
        torch.cuda.synchronize()
        lib.profiler = None
    timer2 = None
    if later and full:
        # the other tagged kernels: the same K steps again (on every rank: a step holds the collective), bracketed, right after
        # the timed region (never part of `value`)
        timer2 = _lib.KernelTimer(only={t for _, t in later.values()}, names={n for n, _ in later.values()})
        lib.profiler = timer2
        for _ in range(args.steps):
            eager_step()
        torch.cuda.synchronize()
        lib.profiler = None
    tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
    if multi is not None:
        # every rank's OWN time for the K steps (the headline is their MAX) and the launch thread's share of it: a slow rank, a slow
        # host or a slow link shows here without a second run
        mine = torch.tensor([dt, t_host], dtype=torch.float64, device=dev)
        allt = [torch.zeros_like(mine) for _ in range(dist.get_world_size())]
        dist.all_gather(allt, mine)
        per = sorted(float(t[0]) / args.steps * 1e3 for t in allt)
        multi["per_rank_ms_per_step"] = {"min": per[0], "median": per[len(per) // 2], "max": per[-1], "by_rank": [float(t[0]) / args.steps * 1e3 for t in allt]}
        multi["per_rank_host_enqueue_ms_per_step"] = [float(t[1]) / args.steps * 1e3 for t in allt]
        if train and full:
            # the collective alone: 20 all-reduces of the flat gradient bucket back to back, HIP events on this rank (a per-link-bound
            # ring over xGMI moves 1.35 MB in tens of microseconds; what is measured here is launch + latency)
            evs = []
            for _ in range(3):
                dist.all_reduce(bucket.flat)
            barrier()
            for _ in range(20):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dist.all_reduce(bucket.flat)
                e1.record()
                evs.append((e0, e1))
            torch.cuda.synchronize()
            us = sorted(a_.elapsed_time(b_) * 1e3 for a_, b_ in evs)
            multi["bucket_all_reduce_us"] = {"bytes": bucket.nbytes, "median": us[len(us) // 2], "min": us[0], "max": us[-1],
                                            "note": "gradient values are scratch after the timed region; launch + ring latency of one all_reduce(sum) of the flat bucket"}
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = float(tmax.item())
    lossv = float(loss)
    # the same K steps with the OTHER weight-gradient mode (the library default is synchronous: what the drop-in runs under the
    # reference's own train.py with DataParallel hooks), reported beside the headline -- never the headline itself
    ms_other_mode = None
    ms_library_default = None
    timer3 = None
    if full and train and not graph_mode and async_wgrad and defer_join:
        # the LIBRARY default (what the drop-in under the reference's own train.py gets): side-stream weight gradients joined INSIDE
        # the regulariser node, so every gradient autograd hands on is finished
        _ops.set_async_wgrad(True, defer_join=False)
        for _ in range(2):
            step()
        barrier()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            step()
        barrier()
        tm = torch.tensor([time.perf_counter() - t1], dtype=torch.float64, device=dev)
        if world > 1:
            dist.all_reduce(tm, op=dist.ReduceOp.MAX)
        ms_library_default = float(tm.item()) / args.steps * 1e3
        _ops.set_async_wgrad(True, defer_join=True)
    ms_split_bf16 = None
    if full and train and not graph_mode:
        # OPT-IN arithmetic (knob conv0_x3 = 3, csrc/conv3d_x3.hip), never the headline: conv0's forward and input gradient on the bf16
        # MFMA with every fp32 operand split into three bf16 terms (six exact products per fp32 product, fp32 accumulation; measured
        # error against fp64 BELOW the fp32-MFMA kernels': tests/test_gpu_parity.py::test_conv0_*_split_bf16_form_vs_fp64)
        import ctypes as _ct
        x3_before = _ct.c_int(0)
        lib.call("mvs_get_tuning", b"conv0_x3", _ct.byref(x3_before))
        lib.call("mvs_set_tuning", b"conv0_x3", 3)
        for _ in range(2):
            step()
        barrier()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            step()
        barrier()
        tm = torch.tensor([time.perf_counter() - t1], dtype=torch.float64, device=dev)
        if world > 1:
            dist.all_reduce(tm, op=dist.ReduceOp.MAX)
        ms_split_bf16 = float(tm.item()) / args.steps * 1e3
        lib.call("mvs_set_tuning", b"conv0_x3", int(x3_before.value))
    ms_join_in_node = None
    if full and train and not graph_mode and async_wgrad and not defer_join and _ops.TAIL_JOIN:
        # what the library default was in rounds 3-5 (MVS_TAIL_JOIN=0): the side stream joined INSIDE the regulariser node
        _ops.TAIL_JOIN = False
        for _ in range(2):
            step()
        barrier()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            step()
        barrier()
        tm = torch.tensor([time.perf_counter() - t1], dtype=torch.float64, device=dev)
        if world > 1:
            dist.all_reduce(tm, op=dist.ReduceOp.MAX)
        ms_join_in_node = float(tm.item()) / args.steps * 1e3
        _ops.TAIL_JOIN = True
    if full and train and not graph_mode:
        _ops.set_async_wgrad(not async_wgrad)
        for _ in range(2):
            step()
        barrier()
        # the roofline kernel again in this pass when it is a weight gradient: with the weight gradients on the main stream it runs
        # ALONE on the GPU (inside the timed region it shares the chip with the main stream's kernels, so its duration there is
        # a statement about the overlap, not about the kernel)
        timer3 = None
        if async_wgrad and dom_key is not None and "wgrad" in dom_key:
            timer3 = _lib.KernelTimer(only={tagmap[dom_key][1]}, names={tagmap[dom_key][0]})
            lib.profiler = timer3
        t1 = time.perf_counter()
        for _ in range(args.steps):
            step()
        barrier()
        lib.profiler = None
        tm = torch.tensor([time.perf_counter() - t1], dtype=torch.float64, device=dev)
        if world > 1:
            dist.all_reduce(tm, op=dist.ReduceOp.MAX)
        ms_other_mode = float(tm.item()) / args.steps * 1e3
        _ops.set_async_wgrad(async_wgrad)
    ms_sustained = None
    if args.sustained > 0:
        # the headline's mode over many more steps with Python's cyclic collector ON (the 20-step headline runs with it disabled)
        import gc as _gc
        _gc.enable()
        for _ in range(2):
            step()
        barrier()
        t1 = time.perf_counter()
        for _ in range(args.sustained):
            step()
        barrier()
        tm = torch.tensor([time.perf_counter() - t1], dtype=torch.float64, device=dev)
        if world > 1:
            dist.all_reduce(tm, op=dist.ReduceOp.MAX)
        ms_sustained = float(tm.item()) / args.sustained * 1e3

    if args.host_profile and rank == 0:
        import cProfile
        import io
        import pstats
        pr = cProfile.Profile()
        barrier()
        pr.enable()
        for _ in range(args.steps):
            step()
        pr.disable()
        barrier()
        buf = io.StringIO()
        st = pstats.Stats(pr, stream=buf)
        st.sort_stats("tottime").print_stats(45)
        st.sort_stats("cumulative").print_stats(60)
        with open(args.host_profile, "w") as fh:
            fh.write("%d steps\n" % args.steps + buf.getvalue())
    ab = {}
    if args.ab and not graph_mode:
        from mvs_amd.jdacs.models.module import ConvBnReLU
        for spec in filter(None, args.ab.split(";")):
            if spec == "defer_join":
                def setter(on, base=defer_join):
                    _ops.set_async_wgrad(async_wgrad, defer_join=(not base) if on else base)
            elif spec.startswith("wgrad_streams="):
                def setter(on, n=int(spec.split("=")[1]), base=args.wgrad_streams):
                    _ops.set_wgrad_streams(n if on else base)
            elif spec == "side_low":
                def setter(on, base=args.side_priority):
                    other = "default" if base == "low" else "low"
                    _ops.set_side_stream_priority(other if on else base)
            elif spec == "side_high":
                def setter(on, base=args.side_priority):
                    _ops.set_side_stream_priority("high" if on else base)
            elif spec == "split_bwd":
                def setter(on, base=ConvBnReLU.split_bwd):
                    ConvBnReLU.split_bwd = (not base) if on else base
            elif spec.startswith("fork_early="):
                def setter(on, n=int(spec.split("=")[1])):
                    _ops._WGRAD_FORK_EARLY = n if on else 0
            elif spec == "feature_one_node":
                from mvs_amd.jdacs.models.mvsnet import FeatureNet as _FN
                def setter(on, base=_FN.one_node):
                    _FN.one_node = (not base) if on else base
            elif spec == "feature_fused_all":
                def setter(on, b1=_ops.FEATURE_FUSED_APPLY, b2=_ops.FEATURE_DGRAD_BNSTATS):
                    _ops.FEATURE_FUSED_APPLY, _ops.FEATURE_DGRAD_BNSTATS = ((True, True) if on else (b1, b2))
            elif spec == "feature_dgrad_bnstats":
                def setter(on, base=_ops.FEATURE_DGRAD_BNSTATS):
                    _ops.FEATURE_DGRAD_BNSTATS = (not base) if on else base
            elif spec == "feature_fused_apply":
                def setter(on, base=_ops.FEATURE_FUSED_APPLY):
                    _ops.FEATURE_FUSED_APPLY = (not base) if on else base
            elif spec == "tail_join":
                def setter(on, base=_ops.TAIL_JOIN):
                    _ops.TAIL_JOIN = (not base) if on else base
            elif spec == "feature_c_entry":
                def setter(on, base=_ops.FEATURE_C_ENTRY):
                    _ops.FEATURE_C_ENTRY = (not base) if on else base
            elif spec == "feature_all_own":
                def setter(on, base=_ops.FEATURE_ALL_OWN):
                    _ops.FEATURE_ALL_OWN = (not base) if on else base
            elif spec == "c_entry":
                def setter(on, base=_ops.C_ENTRY):
                    _ops.C_ENTRY = (not base) if on else base
            elif spec == "feature_bias_side":
                def setter(on, base=_ops.FEATURE_BIAS_SIDE):
                    _ops.FEATURE_BIAS_SIDE = (not base) if on else base
            elif spec == "feature_wgrad_early":
                def setter(on, base=_ops.FEATURE_WGRAD_EARLY):
                    _ops.FEATURE_WGRAD_EARLY = (not base) if on else base
            elif spec == "feature_wgrad_batch":
                def setter(on, base=_ops.FEATURE_WGRAD_BATCH):
                    _ops.FEATURE_WGRAD_BATCH = (not base) if on else base
            elif spec == "feature_dgrad":
                def setter(on, base=ConvBnReLU.hip_dgrad_auto):
                    ConvBnReLU.hip_dgrad_auto = (not base) if on else base
            elif spec == "feature_wgrad":
                def setter(on, base=ConvBnReLU.hip_wgrad):
                    ConvBnReLU.hip_wgrad = (not base) if on else base
            elif spec == "feature_fwd":
                base = ConvBnReLU.hip_fwd_train
                def setter(on, base=base):
                    ConvBnReLU.hip_fwd_train = (not base) if on else base
            else:
                pairs = []     # "key=value[,key=value...]": several knobs toggled together
                for item in spec.split(","):
                    key, _, val = item.partition("=")
                    dflt = _lib.DEFAULT_TUNING.get(key)
                    if dflt is None:       # not in the host-side table: ask the library what it runs with
                        import ctypes
                        cur = ctypes.c_int(0)
                        lib.call("mvs_get_tuning", key.encode(), ctypes.byref(cur))
                        dflt = int(cur.value)
                    pairs.append((key, int(val), dflt))
                def setter(on, pairs=pairs):
                    for key, val, dflt in pairs:
                        lib.call("mvs_set_tuning", key.encode(), val if on else dflt)
            times = ([], [])
            for _ in range(args.ab_reps):
                for on in (0, 1):
                    setter(on)
                    for _ in range(3):
                        step()
                    barrier()
                    t1 = time.perf_counter()
                    for _ in range(args.steps):
                        step()
                    barrier()
                    times[on].append((time.perf_counter() - t1) / args.steps * 1e3)
            setter(0)
            med = [sorted(t)[len(t) // 2] for t in times]
            ab[spec] = {"default_ms": [round(t, 4) for t in times[0]], "toggled_ms": [round(t, 4) for t in times[1]],
                        "median_default_ms": round(med[0], 4), "median_toggled_ms": round(med[1], 4)}
            if rank == 0:
                sys.stderr.write("A/B %s: default %.3f ms/step, toggled %.3f ms/step (medians of %d interleaved runs)\n"
                                 % (spec, med[0], med[1], args.ab_reps))

    if rank == 0:
        summ = timer.summary()
        summ2 = timer2.summary() if timer2 is not None else {}
        kernels = {}
        for key, (name, tag) in tagmap.items():
            if (name, tag) in summ or (name, tag) in summ2:
                calls, ms = summ[(name, tag)] if (name, tag) in summ else summ2[(name, tag)]
                bound, amount = work[key]
                if bound == "hbm":
                    ach, peak, unit = amount / (ms * 1e-3) / 1e9, HBM_PEAK_GBS, "GB/s"
                else:
                    ach, peak, unit = amount / (ms * 1e-3) / 1e12, MFMA_F32_PEAK_TFLOPS, "TFLOP/s"
                kernels[key] = {"bound": bound, "ms": ms, "achieved": ach, "peak": peak, "unit": unit,
                                "frac": ach / peak, "calls": calls,
                                "timed": "HIP events inside the timed region" if (name, tag) in summ
                                else "HIP events, second pass of the same K steps after the timed region"}
        traffic, traffic_note = None, "not collected"
        if full and args.pmc and world == 1:    # tools/pmc_driver.py replays this config's tagged kernels at this config's shapes
            try:
                traffic, traffic_note = pmc_traffic(args.config, dtype)
            except Exception as e:  # the bench line must still come out
                traffic, traffic_note = None, "PMC pass failed: %r" % (e,)
        for k, t in (traffic or {}).items():
            if k in kernels:
                kernels[k]["traffic"] = t["fetch_bytes"] + t["write_bytes"]
                kernels[k]["traffic_fetch"], kernels[k]["traffic_write"] = t["fetch_bytes"], t["write_bytes"]
                kernels[k]["hip_kernel"] = t.get("hip_kernel")
                if "sq" in t:
                    # a second bound for the kernel: the time its vector-ALU instructions need at one wave-instruction per 4 cycles
                    # and SIMD (clock from the same counter pass); `frac_of_valu_issue_ceiling` = that time / the measured duration
                    sq = dict(t["sq"])
                    if sq.get("valu_issue_frac"):
                        sq["valu_issue_floor_ms"] = kernels[k]["ms"] * sq["valu_issue_frac"]     # (the fraction is of the profiled launch)
                    if sq.get("valu_issue_frac") and work[k][0] == "hbm":
                        sq["bound_note"] = ("vector-ALU issue + latency bound: `frac` (of the HBM peak) is the distance to a roof this kernel "
                                            "cannot reach; `valu_issue_frac` = share of the kernel's cycles its SIMDs' issue ports are taken by "
                                            "vector-ALU instructions")
                    kernels[k]["sq_counters"] = sq
                # bytes each launch has to move at least once (conv: input volume + output volume, fp32)
                if work[k][0] == "hbm":
                    kernels[k]["algorithmic_bytes"] = work[k][1]
                elif k.startswith("conv0"):
                    kernels[k]["algorithmic_bytes"] = (FEAT_C + 8) * ndepth * (img_h // 4) * (img_w // 4) * 4
                elif k in ("conv_64_64", "conv_16_16"):
                    cch = 64 if k == "conv_64_64" else 16
                    kernels[k]["algorithmic_bytes"] = int(work[k][1] // (27 * cch)) * 4   # = 2 * cch * voxels * 4
        # the roofline object describes the dominant (longest-running) kernel of the step; the other tagged kernels are in "kernels"
        if timer3 is not None:
            s3 = timer3.summary().get(tagmap[dom_key])
            if s3 and dom_key in kernels:
                k3 = kernels[dom_key]
                k3["ms_alone"] = s3[1]
                k3["frac_alone"] = work[dom_key][1] / (s3[1] * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS
                k3["alone_is"] = ("the same launch in the synchronous-weight-gradient pass after the timed region (main stream, nothing "
                                  "beside it); `ms` / `frac` are its duration on the side stream, under the main stream's kernels")
        if full and dom_key == "conv0_wgrad" and dom_key in kernels and train and world == 1:
            try:
                kernels[dom_key].update(wgrad_all_cus(lib, dev, (ndepth, img_h // 4, img_w // 4), work[dom_key][1]))
            except Exception as e:  # the bench line must still come out
                kernels[dom_key]["all_cus_is"] = "not measured: %r" % (e,)
        dom = max(kernels, key=lambda k: kernels[k]["ms"], default=None)
        roof = None
        if dom is not None:
            roof = {"kernel": dom, "hip_kernel": HIP_KERNEL_OF[dom], "bound": kernels[dom]["bound"], "achieved": kernels[dom]["achieved"],
                    "peak": kernels[dom]["peak"], "unit": kernels[dom]["unit"], "frac": kernels[dom]["frac"],
                    "traffic": kernels[dom].get("traffic"), "traffic_unit": "bytes of HBM traffic per launch", "traffic_source": traffic_note,
                    "ms": kernels[dom]["ms"], "timed": kernels[dom]["timed"]}
            for extra in ("ms_alone", "frac_alone", "alone_is", "ms_all_cus", "frac_all_cus", "groups_in_step", "all_cus_is", "sq_counters"):
                if extra in kernels[dom]:
                    roof[extra] = kernels[dom][extra]
        metric = {2: "depth-samples/sec (N=3, 640x512, D=192)", 3: "depth-samples/sec (JDACS self-supervised step, N=5, 640x512, D=192)",
                  4: "depth-samples/sec (CVP-MVSNet 3-level inference, N=5, 1152x864, D=(48,8,8))",
                  5: "depth-samples/sec (MVSNet inference, N=7, 1600x1184, D=256)"}[args.config]
        res = {
            "metric": metric, "value": world * max(1, args.batch) * args.steps / dt,
            "unit": "depth-samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": dtype, "data": "synthetic",
            "config": {"workload": cfg["what"], "baseline_config_index": args.config - 1,
                       "views": nviews, "image": [img_h, img_w], "depth_planes": ndepth,
                       "global_batch": world * max(1, args.batch), "samples_per_gpu_per_step": max(1, args.batch), "parallelism": "dp%d" % world},
            "ranks": (dist.get_world_size() if world > 1 else 1), "multi_gpu": multi,
            "collective": ("RCCL all_reduce(sum) of one flat fp32 bucket, %d ranks%s" % (world, " (--force-collective)" if world == 1 else ""))
            if ((world > 1 or args.force_collective) and train) else "none",
            "roofline": roof, "kernels": kernels, "final_loss": lossv,
            "launch_mode": "hipGraph replay" if graph_mode else "eager",
            "async_wgrad": bool(async_wgrad) if train else None, "async_wgrad_is_library_default": bool(_ops.FUSED_REGULARISER),
            "fused_regulariser_node": bool(_ops.FUSED_REGULARISER),
            "wgrad_join": ("end of backward pass (opt-in engine callback, ops.set_async_wgrad(defer_join=True))" if defer_join else
                           ("end of backward pass (library default: MVSNet's tail node, ops.DeferredJoinFn)" if (_ops.TAIL_JOIN and async_wgrad and args.config in (2, 3))
                            else "inside the regulariser node")) if train else None,
            "headline_mode_is_library_default": bool(async_wgrad and not defer_join) if train else None,
            "host_enqueue_ms_per_step": t_host / args.steps * 1e3, "allocator_in_timed_region": alloc_diag,
            "host_enqueue_ms_per_step_median_max": [host_steps[len(host_steps) // 2], host_steps[-1]], "wgrad_streams": args.wgrad_streams, "side_stream_priority": args.side_priority,
            ("ms_per_step_async_wgrad_off" if async_wgrad else "ms_per_step_async_wgrad_on"): ms_other_mode,
            "ms_per_step_library_default": (ms_library_default if (async_wgrad and defer_join) else (dt / args.steps * 1e3 if async_wgrad else ms_other_mode)) if train else None,
            "ms_per_step_join_inside_regulariser_node": ms_join_in_node,
            "ms_per_step_opt_in_split_bf16_conv0": ms_split_bf16,
            "opt_in_split_bf16_is": "the same K steps with mvs_set_tuning('conv0_x3', 3): conv0's forward and input gradient as six bf16 MFMA "
                                    "products of three-term splits of the fp32 operands, fp32 accumulation (csrc/conv3d_x3.hip; its weight "
                                    "gradient stays on the fp32 MFMA). NOT the headline and not the default: `value`, `ms_per_step` and `dtype` "
                                    "are the all-fp32-MFMA step" if ms_split_bf16 else None,
            "library_default_is": "MVS_ASYNC_WGRAD unset, no set_async_wgrad call: side-stream weight gradients, joined by MVSNet's tail node at the "
                                  "end of the backward pass (MVS_TAIL_JOIN=0: inside the regulariser node, rounds 3-5)",
            "grad_bucket_bytes": bucket.nbytes if bucket is not None else 0,
            "full": full,
        }
        if ms_sustained is not None:
            res["ms_per_step_sustained"] = ms_sustained
            res["sustained_steps"] = args.sustained
        if full and cfg["kind"] == "cvp_infer":
            # the 2-D feature pyramid (jdacs-ms/models/network.py:16-41: nine 3x3 convolutions per image, at the three resolutions of
            # this config, N images): its algorithmic FLOPs, the time of its C-ABI calls (HIP events, one more pass of the K steps)
            # and its share of the step
            from mvs_amd.jdacs_ms.models.network import _PYRAMID_LAYERS
            macs_per_px = sum(9 * cin * cout for _, cin, cout in _PYRAMID_LAYERS)
            px = sum((img_h >> lv) * (img_w >> lv) for lv in range(3)) * nviews
            t_py = _lib.KernelTimer(None)
            lib.profiler = t_py
            for _ in range(args.steps):
                eager_step()
            torch.cuda.synchronize()
            lib.profiler = None
            py_ms = sum(ms * c for (n, t), (c, ms) in t_py.summary().items() if n.startswith("mvs_conv2d")) / args.steps
            res["feature_pyramid"] = {"gflop_per_step": 2.0 * macs_per_px * px / 1e9, "ms_per_step": py_ms,
                                      "share_of_step": py_ms / (dt / args.steps * 1e3),
                                      "achieved_tflops": 2.0 * macs_per_px * px / (py_ms * 1e-3) / 1e12 if py_ms else None,
                                      "frac_of_mfma_peak": 2.0 * macs_per_px * px / (py_ms * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS if py_ms else None,
                                      "timed": "HIP events around every mvs_conv2d* call, a pass of the same K steps after the timed region"}
        if ab:
            res["ab"] = ab
        if host_trace is not None:
            os.makedirs("gpurun_out", exist_ok=True)
            with open("gpurun_out/host_trace.json", "w") as f:
                json.dump({"marks": host_marks, "rows": host_trace.rows}, f)
        if step_events:
            res["warmup_enqueue_ms"], res["opening_barrier_wait_ms"] = round(t_warm * 1e3, 2), round(t_gap * 1e3, 2)
            res["step_gpu_ms"] = [round(a.elapsed_time(b), 3) for a, b in zip(step_events, step_events[1:])]
            res["step_host_ms"] = [round((b - a) * 1e3, 3) for a, b in zip(host_marks, host_marks[1:])]
            if train and join_trace:
                # > 0: the side stream (weight gradients) finishes after the main stream's backward pass and the join waits for it
                lag = sorted(em.elapsed_time(es) for em, es in join_trace)
                res["side_stream_lag_at_join_ms_median_max"] = [round(lag[len(lag) // 2], 3), round(lag[-1], 3)]
            if train:
                res["step_host_fwd_bwd_rest_ms"] = [[round((phase_marks[2 * i] - host_marks[i]) * 1e3, 2),
                                                      round((phase_marks[2 * i + 1] - phase_marks[2 * i]) * 1e3, 2),
                                                      round((host_marks[i + 1] - phase_marks[2 * i + 1]) * 1e3, 2)] for i in range(args.steps)][:6]
        if full and not args.no_cpu_baseline and world == 1 and args.config == 2:   # rank 0 at N=1 only (bench contract)
            try:
                res["cpu_baseline"] = cpu_baseline(state0, 1)
            except Exception as e:  # the bench line must still come out
                res["cpu_baseline"] = {"value": None, "error": repr(e)}
        want_ref = args.gpu_reference == 1 or (args.gpu_reference < 0 and full and world == 1 and args.config == 2 and not args.no_cpu_baseline)
        if want_ref and args.config == 2:
            try:
                from oracle import ref_torch as R
                old_sampler = R.set_sampler("aten")   # F.grid_sample as the reference calls it (module.py:136)
                oracle = R.OracleMVSNet(refine=False)
                oracle.load_state_dict(state0)
                oracle = oracle.to(dev).train()
                oopt = torch.optim.Adam(oracle.parameters(), lr=1e-4)

                def ostep():
                    oopt.zero_grad(set_to_none=True)
                    o = oracle(imgs, proj, dv)
                    R.mvsnet_loss(o["depth"], gt, mask).backward()
                    oopt.step()
                for _ in range(3):
                    ostep()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(5):
                    ostep()
                torch.cuda.synchronize()
                odt = (time.perf_counter() - t1) / 5
                res["reference_gpu_path"] = {"value": 1.0 / odt, "unit": "depth-samples/s", "ms_per_step": odt * 1e3,
                                             "what": "oracle/ref_torch.py with sampler='aten' (stock PyTorch-ROCm ops: ATen grid_sample, "
                                                     "MIOpen conv3d / batch_norm, cudnn.benchmark on) on the same MI355X, same step",
                                             "speedup": (world * args.steps / dt) * odt}
                del oracle, oopt
                torch.cuda.empty_cache()
            except Exception as e:
                res["reference_gpu_path"] = {"value": None, "error": repr(e)}
            finally:
                R.set_sampler("gather")
        if args.torch_profile:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                for _ in range(5):
                    eager_step()
                torch.cuda.synchronize()
            with open(args.torch_profile, "w") as fh:
                fh.write(prof.key_averages().table(sort_by="cuda_time_total", row_limit=70, max_name_column_width=90))
                fh.write("\n\n")
                fh.write(prof.key_averages().table(sort_by="cpu_time_total", row_limit=40, max_name_column_width=90))
        if args.time_all_kernels:
            t_all = _lib.KernelTimer(None)
            lib.profiler = t_all
            for _ in range(3):
                eager_step()
            torch.cuda.synchronize()
            lib.profiler = None
            rows = sorted(((ms * c / 3.0, n, t, c // 3, ms) for (n, t), (c, ms) in t_all.summary().items()), reverse=True)
            tot = sum(r[0] for r in rows)
            sys.stderr.write("---- per-step kernel time by C-ABI call (HIP events), total %.3f ms ----\n" % tot)
            for r in rows:
                sys.stderr.write("%8.3f ms/step  x%d  %8.3f ms  %-32s %s\n" % (r[0], r[3], r[4], r[1], r[2]))
        emit(json.dumps(res))
    if world > 1:
        dist.barrier()
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
