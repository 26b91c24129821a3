#!/usr/bin/env python3
"""Generate tests/golden/g13_*.npz by EXECUTING the reference's own modules (build container only): the wider cases of
tests/test_oracle_vs_reference.py -- more views, align_corners=True (the authors' torch-1.1 behaviour, App. A Q1), a
3-level CVP, UnSupLoss at N = 7 and the bytes of save_pfm.

    python tests/golden/make_golden_vs_reference.py

Each case runs in a fresh interpreter (jdacs and jdacs-ms both own a top-level `models` package).  Only tensors are stored:
the reference's outputs and gradients for the seeded inputs the test regenerates, per-tensor sums of the reference's initial
weights (the test rebuilds the same weights from the same seed and checks those sums first) and the PFM file's bytes.  The
gradients of the larger models are split over several files so that every fixture stays below 1 MiB."""
import os
import subprocess
import sys
import warnings

sys.dont_write_bytecode = True
warnings.filterwarnings("ignore")

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"


def _setup(sub):
    sys.path.insert(0, ROOT)
    sys.argv = ["x"]
    sys.path.insert(0, os.path.join(REF, sub))
    import torch
    torch.set_num_threads(4)
    return torch


def _save(name, arrays):
    import numpy as np
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in arrays.items()})
    print(name, len(arrays), "arrays", os.path.getsize(path), "bytes")


def _save_split(name, head, grads, budget=800_000):
    """head + gradient tensors in <name>_a, <name>_b, ...: each file's raw payload below `budget` bytes"""
    parts, cur, size = [], dict(head), sum(v.nbytes for v in head.values())
    for k, v in grads.items():
        if size + v.nbytes > budget and len(cur):
            parts.append(cur)
            cur, size = {}, 0
        cur["grad." + k] = v
        size += v.nbytes
    parts.append(cur)
    for i, part in enumerate(parts):
        _save("%s_%s" % (name, "abcdefgh"[i]), part)


def _sd_sums(model):
    return {"sdsum." + k: v.double().sum().numpy() for k, v in model.state_dict().items()}


def case_mvsnet():
    torch = _setup("jdacs")
    from oracle import ref_torch as R
    from models.mvsnet import MVSNet
    torch.manual_seed(0)
    ref = MVSNet(refine=True)
    with torch.no_grad():
        ref.cost_regularization.prob.weight.mul_(50.0)
    head = _sd_sums(ref)
    imgs, proj, dv = R.synthetic_mvsnet_inputs(2, 5, 64, 96, 16, seed=3)
    ref.train()
    a = ref(imgs, proj, dv)
    head.update({"train_depth": a["depth"].detach().numpy(), "train_conf": a["photometric_confidence"].detach().numpy()})
    a["depth"].mean().backward()
    grads = {k: p.grad.numpy() for k, p in ref.named_parameters() if p.grad is not None}
    ref.eval()
    with torch.no_grad():
        a = ref(imgs, proj, dv)
    head.update({"eval_depth": a["depth"].numpy(), "eval_conf": a["photometric_confidence"].numpy()})
    _save_split("g13_mvsnet_five_views", head, grads)


def case_warp():
    torch = _setup("jdacs")
    import torch.nn.functional as F
    from oracle import ref_torch as R
    from models import module as refmod
    _gs = F.grid_sample
    refmod.F.grid_sample = lambda inp, grid, **kw: _gs(inp, grid, align_corners=True, **kw)  # torch-1.1 semantics
    imgs, proj, dv = R.synthetic_mvsnet_inputs(2, 3, 48, 64, 8, seed=5)
    src = torch.randn(2, 8, 12, 16, generator=torch.Generator().manual_seed(6))
    out = refmod.homo_warping(src, proj[:, 1].contiguous(), proj[:, 0].contiguous(), dv)
    _save("g13_homo_warping_align_corners", {"src": src.numpy(), "out": out.numpy()})


def case_cvp():
    torch = _setup("jdacs-ms")
    import types
    from oracle import ref_torch as R
    torch.Tensor.cuda = lambda self, *a, **k: self
    from models.network import CVPMVSNet
    torch.manual_seed(0)
    args = types.SimpleNamespace(nsrc=3, nscale=3, mode="train")
    ref = CVPMVSNet(args)
    ref.train()
    head = _sd_sums(ref)
    g = torch.Generator().manual_seed(2)
    ih, iw = 96, 128
    K, E = R.synthetic_cameras(4, ih, iw, iw)
    ins = [torch.randn(1, 3, ih, iw, generator=g), torch.randn(1, 3, 3, ih, iw, generator=g), K.unsqueeze(0),
           K.view(1, 1, 3, 3).repeat(1, 3, 1, 1), E[0].unsqueeze(0), E[1:].unsqueeze(0), torch.tensor([425.0]),
           torch.tensor([425.0 + 47 * 13.5])]
    a = ref(*ins)
    for i, d in enumerate(a["depth_est_list"]):
        head["depth_%d" % i] = d.detach().numpy()
    head["prob_confidence"] = a["prob_confidence"].detach().numpy()
    sum(d.mean() for d in a["depth_est_list"]).backward()
    grads = {k: p.grad.numpy() for k, p in ref.named_parameters() if p.grad is not None}
    _save_split("g13_cvpmvsnet_three_levels", head, grads)


def case_unsup():
    torch = _setup("jdacs")
    import importlib.util
    import tempfile
    import numpy as np
    import torch.nn.functional as F
    from oracle import ref_torch as R
    sys.argv = ["x", "--smooth_lambda", "0.5"]
    from losses.unsup_loss import UnSupLoss
    g = torch.Generator().manual_seed(4)
    b, n, h, w = 3, 7, 52, 76
    imgs = F.avg_pool2d(torch.randn(b * n, 3, h, w, generator=g), 5, 1, 2).view(b, n, 3, h, w) * 3
    K, E = R.synthetic_cameras(n, h // 4, w // 4, w)
    cams = torch.zeros(b, n, 2, 4, 4)
    cams[:, :, 0] = E
    cams[:, :, 1, :3, :3] = K
    depth = (600.0 + 40.0 * torch.rand(b, h // 4, w // 4, generator=g)).requires_grad_(True)
    loss = UnSupLoss()(imgs, cams, depth)
    loss.backward()
    spec = importlib.util.spec_from_file_location("ref_data_io", os.path.join(REF, "jdacs", "datasets", "data_io.py"))
    ref_io = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_io)
    arr = np.random.RandomState(1).rand(17, 23).astype(np.float32) * 900
    with tempfile.TemporaryDirectory() as d:
        ref_io.save_pfm(os.path.join(d, "a.pfm"), arr)
        raw = open(os.path.join(d, "a.pfm"), "rb").read()
        back = ref_io.read_pfm(os.path.join(d, "a.pfm"))[0]
    _save("g13_unsup_loss_seven_views", {"loss": loss.detach().numpy(), "depth_grad": depth.grad.numpy(),
                                         "pfm_array": arr, "pfm_bytes": np.frombuffer(raw, dtype=np.uint8),
                                         "pfm_read_back": np.ascontiguousarray(back)})


CASES = {"mvsnet": case_mvsnet, "warp": case_warp, "cvp": case_cvp, "unsup": case_unsup}

if __name__ == "__main__":
    if len(sys.argv) > 1:
        CASES[sys.argv[1]]()
    else:
        for name in CASES:
            subprocess.run([sys.executable, os.path.abspath(__file__), name], check=True, cwd=ROOT,
                           env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
