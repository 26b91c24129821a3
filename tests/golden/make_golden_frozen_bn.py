#!/usr/bin/env python3
"""Generate tests/golden/g18_frozen_bn_mvs*.npz and g18_frozen_bn_cvp*.npz by IMPORTING the reference (build container only).

    python tests/golden/make_golden_frozen_bn.py

Fine-tuning with FROZEN BatchNorm statistics, the way PyTorch users do it: ``model.train()``, then ``.eval()`` on every BatchNorm
module.  The live jdacs ``MVSNet(refine=False)`` gets g6_mvsnet_e2e.npz's weights (``sd.*``) and calibrated running statistics
(``cal.*``) and runs on g6's inputs; the live jdacs-ms ``CVPMVSNet`` gets g7_cvpmvsnet_e2e.npz's weights and inputs (g7 carries no
running statistics: two calibration forwards with BatchNorm momentum 1 produce them, and they are stored as ``cal.*``).  Inputs and
weights are READ from g6 / g7, not duplicated.  Stored: depth, the regulariser's logits, every parameter gradient and the image
gradient (fp32) of loss = mean(depth * linspace(0.5, 1.5)) (summed over the levels for CVP), and the running statistics after the
step (``after.*`` -- they must be the ones before it).

No committed file may exceed 1 MiB and fp32 gradients hardly compress, so a fixture is written as one or a few part files
(``<name>.npz``, ``<name>_b.npz``, ...) with disjoint keys; tests/frozen_bn_cases.py:load_parts merges them."""
import os
import sys
import types
import warnings
import zlib

sys.dont_write_bytecode = True
warnings.filterwarnings("ignore")
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.argv = ["x"]
torch.set_num_threads(4)
PART_BYTES = 900 * 1024


def load(name):
    z = np.load(os.path.join(HERE, name + ".npz"))
    out = {}
    for k in z.files:
        t = torch.from_numpy(z[k])
        out[k] = t.float() if z[k].dtype == np.float16 else t
    return out


def save_parts(name, arrs):
    """disjoint key sets, each part below PART_BYTES of compressed payload (estimated per array)"""
    parts, cur, size = [], {}, 0
    for k, v in arrs.items():
        v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        nbytes = len(zlib.compress(v.tobytes())) + 256
        assert nbytes < PART_BYTES, k
        if cur and size + nbytes > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += nbytes
    parts.append(cur)
    for i, part in enumerate(parts):
        path = os.path.join(HERE, name + ("" if i == 0 else "_" + "abcdefgh"[i]) + ".npz")
        np.savez_compressed(path, **part)
        assert os.path.getsize(path) < (1 << 20), path
        print("%-34s %8.1f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))


def freeze_batchnorm(net):
    net.train()
    for m in net.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.eval()


def weighted_mean(depth):
    return (depth * torch.linspace(0.5, 1.5, depth.numel()).view_as(depth)).mean()


def check(depths, grads):
    for d in depths:
        assert float(d.std()) > 0.0, "degenerate depth map"
    for k, v in grads.items():
        assert v is not None and float(v.abs().max()) > 0.0, "all-zero gradient: " + k


def buffers(net):
    return {"after." + k: v.clone() for k, v in net.state_dict().items() if "running" in k or "num_batches" in k}


# =============================================================================================
# jdacs (MVSNet backbone) on g6
# =============================================================================================
sys.path.insert(0, os.path.join(REF, "jdacs"))
from models.mvsnet import MVSNet  # noqa: E402

g6 = load("g6_mvsnet_e2e")
net = MVSNet(refine=False)
sd = {k[3:]: v for k, v in g6.items() if k.startswith("sd.")}
sd.update({k[4:]: v for k, v in g6.items() if k.startswith("cal.")})
net.load_state_dict(sd)
freeze_batchnorm(net)
before = buffers(net)
cap = {}
net.cost_regularization.register_forward_hook(lambda m, i, o: cap.update(logits=o.detach().clone()))
imgs = g6["imgs"].clone().requires_grad_(True)
out = net(imgs, g6["proj"], g6["depth_values"])
weighted_mean(out["depth"]).backward()
grads = {"grad." + k: p.grad for k, p in net.named_parameters() if not k.endswith("prob.bias")}
grads["grad_imgs"] = imgs.grad
check([out["depth"]], grads)
after = buffers(net)
assert all(torch.equal(before[k], after[k]) for k in before)
grads["grad." + "cost_regularization.prob.bias"] = net.cost_regularization.prob.bias.grad      # (exactly zero: d softmax / d bias)
save_parts("g18_frozen_bn_mvs", dict(depth=out["depth"], conf=out["photometric_confidence"], logits=cap["logits"], **after, **grads))

# =============================================================================================
# jdacs-ms (CVP-MVSNet backbone) on g7
# =============================================================================================
for m in [k for k in list(sys.modules) if k.split(".")[0] in ("models", "losses", "utils", "config", "datasets")]:
    del sys.modules[m]
sys.path[0] = os.path.join(REF, "jdacs-ms")
torch.Tensor.cuda = lambda self, *a, **k: self  # the reference's modules hard-code .cuda()
from models.network import CVPMVSNet  # noqa: E402

g7 = load("g7_cvpmvsnet_e2e")
args = types.SimpleNamespace(nsrc=2, nscale=2, mode="train")
cvp = CVPMVSNet(args)
cvp.load_state_dict({k[3:]: v for k, v in g7.items() if k.startswith("sd.")}, strict=False)
ins = [g7[k] for k in ("ref_img", "src_imgs", "ref_in", "src_in", "ref_ex", "src_ex", "depth_min", "depth_max")]
bns = [m for m in cvp.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
cvp.train()
for m in bns:
    m.momentum = 1.0
with torch.no_grad():
    for _ in range(2):
        cvp(*ins)
for m in bns:
    m.momentum = 0.1
cal = {"cal." + k: v.clone() for k, v in cvp.state_dict().items() if "running" in k or "num_batches" in k}
freeze_batchnorm(cvp)
before = buffers(cvp)
logits = []
cvp.cost_reg_refine.register_forward_hook(lambda m, i, o: logits.append(o.detach().clone()))
ref_img, src_imgs = ins[0].clone().requires_grad_(True), ins[1].clone().requires_grad_(True)
out = cvp(ref_img, src_imgs, *ins[2:])
depths = out["depth_est_list"]
sum(weighted_mean(d) for d in depths).backward()
grads = {"grad." + k: p.grad for k, p in cvp.named_parameters() if not k.endswith("prob0.bias")}
grads["grad_ref_img"], grads["grad_src_imgs"] = ref_img.grad, src_imgs.grad
check(depths, grads)
after = buffers(cvp)
assert all(torch.equal(before[k], after[k]) for k in before)
grads["grad.cost_reg_refine.prob0.bias"] = cvp.cost_reg_refine.prob0.bias.grad
save_parts("g18_frozen_bn_cvp", dict(depth0=depths[0], depth1=depths[1], conf=out["prob_confidence"],
                                      **{"logits%d" % i: t for i, t in enumerate(logits)}, **cal, **after, **grads))
print("done")
