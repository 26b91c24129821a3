#!/usr/bin/env python3
"""Timing evidence for fine-tuning with frozen BatchNorm statistics on one GPU, at BASELINE config 2's step (MVSNet, N = 3 views of
640 x 512, D = 192, mvsnet_loss): zero the gradients, forward, loss, backward -- no optimiser step, so every repetition sees the
same parameters --
  (a) train mode, as it stands (batch statistics, the one-node regulariser and extractor);
  (b) the freeze idiom (model.train(), every BatchNorm module .eval()) on the frozen path: ops.UNetRegulariserFrozenFn, the 2-D
      blocks through ops.BnReLUFn(training=False);
  (c) the freeze idiom on the oracle's stock PyTorch-ROCm modules (oracle/ref_torch.py:OracleMVSNet) on the same GPU.
The running statistics are calibrated first (one train-mode forward with momentum 1), so (b) and (c) normalise with meaningful
values.  The three are INTERLEAVED -- one repetition of each per round, torch.cuda.Event pairs around each -- after 5 warm-up rounds,
25 rounds; reported are the median and the 10th / 90th percentiles.  (b)'s depth map is compared with (c)'s, and the running
statistics are checked to be untouched by (b).
Writes one JSON object to profiles/frozen_bn_timing.json and prints it."""
import json
import os
import sys

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")      # the oracle's stock convolutions: no exhaustive search at this size
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import mvs_amd  # noqa: F401
from mvs_amd.jdacs.models.mvsnet import MVSNet, mvsnet_loss
from mvs_amd.synthetic import synthetic_mvsnet_inputs
from oracle import ref_torch as R

ROUNDS, WARMUP = 25, 5
NVIEWS, IMG_H, IMG_W, NDEPTH = 3, 512, 640, 192
dev = torch.device("cuda:0")
_BN = torch.nn.modules.batchnorm._BatchNorm


def freeze_batchnorm(net):
    net.train()
    for m in net.modules():
        if isinstance(m, _BN):
            m.eval()
    return net


def calibrate(net, *inputs):
    bns = [m for m in net.modules() if isinstance(m, _BN)]
    for m in bns:
        m.momentum = 1.0
    net.train()
    with torch.no_grad():
        net(*inputs)
    for m in bns:
        m.momentum = 0.1


def summary(ms):
    ms = sorted(ms)
    q = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]
    return {"median_ms": q(0.5), "p10_ms": q(0.1), "p90_ms": q(0.9), "rounds": ROUNDS, "warmup": WARMUP}


torch.manual_seed(0)
net_a = MVSNet(refine=False)
with torch.no_grad():
    net_a.cost_regularization.prob.weight.mul_(50.0)
net_a = net_a.to(dev)
imgs, proj, dv = (t.to(dev) for t in synthetic_mvsnet_inputs(1, NVIEWS, IMG_H, IMG_W, NDEPTH, seed=1))
gt = torch.full((1, IMG_H // 4, IMG_W // 4), 650.0, device=dev)
mask = torch.ones_like(gt)
calibrate(net_a, imgs, proj, dv)
net_b = MVSNet(refine=False)
net_b.load_state_dict(net_a.state_dict())
net_b = freeze_batchnorm(net_b.to(dev))
net_c = R.OracleMVSNet(refine=False)
net_c.load_state_dict(net_a.state_dict())
net_c = freeze_batchnorm(net_c.to(dev))
net_a.train()
stats_before = {k: v.clone() for k, v in net_b.state_dict().items() if "running" in k or "num_batches" in k}
last = {}


def step(tag, net, loss_fn):
    def run():
        net.zero_grad(set_to_none=True)
        out = net(imgs, proj, dv)
        loss_fn(out["depth"], gt, mask).backward()
        last[tag] = out["depth"].detach()
    return run


steps = [("a_train_mode", step("a", net_a, mvsnet_loss)), ("b_frozen_hip", step("b", net_b, mvsnet_loss)),
         ("c_frozen_stock_ops", step("c", net_c, R.mvsnet_loss))]
times = {name: [] for name, _ in steps}
for r in range(WARMUP + ROUNDS):
    for name, fn in steps:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if r >= WARMUP:
            times[name].append(e0.elapsed_time(e1))
untouched = all(torch.equal(v, net_b.state_dict()[k]) for k, v in stats_before.items())
rel = float((last["b"] - last["c"]).abs().mean() / last["c"].abs().mean())
grads_finite = all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net_b.parameters())
res = {"what": "BASELINE config-2 step (MVSNet N=3, 640x512, D=192, mvsnet_loss; zero_grad + forward + loss + backward, no optimiser "
               "step): (a) train mode, (b) freeze idiom on the frozen-statistics HIP path, (c) freeze idiom on the oracle's stock "
               "PyTorch-ROCm ops; interleaved rounds",
       "device": torch.cuda.get_device_name(0),
       "b_running_statistics_untouched": bool(untouched), "b_gradients_finite": bool(grads_finite),
       "depth_rel_l1_b_vs_c": rel}
for name, _ in steps:
    res[name] = summary(times[name])
res["ratio_b_over_a_median"] = res["b_frozen_hip"]["median_ms"] / res["a_train_mode"]["median_ms"]
res["ratio_c_over_b_median"] = res["c_frozen_stock_ops"]["median_ms"] / res["b_frozen_hip"]["median_ms"]
out_dir = os.path.join(ROOT, "profiles")
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "frozen_bn_timing.json"), "w") as fh:
    json.dump(res, fh, indent=1)
    fh.write("\n")
print(json.dumps(res))
