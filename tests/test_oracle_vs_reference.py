"""The oracle against what the reference's own Python computed (tests/golden/g13_*.npz, written by
tests/golden/make_golden_vs_reference.py, which executes the reference's modules).  CPU only.  Wider cases than the other
goldens: more views, align_corners=True (the authors' torch-1.1 behaviour, App. A Q1), 3-level CVP, UnSupLoss at N = 7."""
import glob
import os
import sys
import tempfile
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import ref_torch as R  # noqa: E402


@pytest.fixture(autouse=True)
def _four_threads():
    """the thread count the fixtures were generated with (the summation order of the CPU kernels follows it)"""
    old = torch.get_num_threads()
    torch.set_num_threads(4)
    yield
    torch.set_num_threads(old)


def _fixture(name):
    """every part of a fixture (<name>.npz, or <name>_a.npz, <name>_b.npz, ... when split to keep files small) as tensors"""
    paths = sorted(glob.glob(os.path.join(GOLDEN, name + "_?.npz"))) or [os.path.join(GOLDEN, name + ".npz")]
    out = {}
    for p in paths:
        z = np.load(p)
        out.update((k, torch.from_numpy(z[k])) for k in z.files)
    return out


def _assert_reference_weights(model, g):
    """the model was built from the seed the reference's model was built from: its initial tensors are the reference's"""
    for k, v in model.state_dict().items():
        assert float(v.double().sum()) == float(g["sdsum." + k]), k


def test_mvsnet_five_views_train_and_eval():
    g = _fixture("g13_mvsnet_five_views")
    torch.manual_seed(0)
    ora = R.OracleMVSNet(refine=True)
    with torch.no_grad():
        ora.cost_regularization.prob.weight.mul_(50.0)
    _assert_reference_weights(ora, g)
    imgs, proj, dv = R.synthetic_mvsnet_inputs(2, 5, 64, 96, 16, seed=3)
    for mode in ("train", "eval"):
        getattr(ora, mode)()
        b = ora(imgs, proj, dv)
        assert torch.allclose(g[mode + "_depth"], b["depth"], rtol=1e-5, atol=1e-3), mode
        assert torch.allclose(g[mode + "_conf"], b["photometric_confidence"], atol=1e-4), mode
        if mode == "train":
            b["depth"].mean().backward()
            for k, q in ora.named_parameters():
                if q.grad is None or k.endswith("prob.bias"):
                    continue
                p = g["grad." + k]
                assert float((p - q.grad).abs().mean()) <= 2e-3 * float(p.abs().mean()) + 1e-9, k


def test_homo_warping_align_corners_true():
    g = _fixture("g13_homo_warping_align_corners")
    imgs, proj, dv = R.synthetic_mvsnet_inputs(2, 3, 48, 64, 8, seed=5)
    src = torch.randn(2, 8, 12, 16, generator=torch.Generator().manual_seed(6))
    assert torch.equal(src, g["src"])
    sp, rp = proj[:, 1].contiguous(), proj[:, 0].contiguous()
    b = R.homo_warping(src, sp, rp, dv, align_corners=True)
    assert float((g["out"] - b).abs().max()) < 2e-5


def test_cvpmvsnet_three_levels():
    g = _fixture("g13_cvpmvsnet_three_levels")
    torch.manual_seed(0)
    args = types.SimpleNamespace(nsrc=3, nscale=3, mode="train")
    ora = R.OracleCVPMVSNet(args)
    ora.train()
    _assert_reference_weights(ora, g)
    gen = torch.Generator().manual_seed(2)
    ih, iw = 96, 128
    K, E = R.synthetic_cameras(4, ih, iw, iw)
    ins = [torch.randn(1, 3, ih, iw, generator=gen), torch.randn(1, 3, 3, ih, iw, generator=gen), K.unsqueeze(0),
           K.view(1, 1, 3, 3).repeat(1, 3, 1, 1), E[0].unsqueeze(0), E[1:].unsqueeze(0), torch.tensor([425.0]),
           torch.tensor([425.0 + 47 * 13.5])]
    b = ora(*ins)
    assert len(b["depth_est_list"]) == len([k for k in g if k.startswith("depth_")])
    for i, y in enumerate(b["depth_est_list"]):
        x = g["depth_%d" % i]
        assert float((x - y).abs().mean() / y.abs().mean()) < 1e-5   # fp32 roundoff chained through 3 levels of batch-stat BN
        assert torch.allclose(x, y, rtol=1e-4, atol=5e-2)
    assert torch.allclose(g["prob_confidence"], b["prob_confidence"], atol=1e-4)
    sum(d.mean() for d in b["depth_est_list"]).backward()
    for k, q in ora.named_parameters():
        if q.grad is None or k.endswith("prob0.bias"):
            continue
        p = g["grad." + k]
        assert float((p - q.grad).abs().mean()) <= 3e-2 * float(p.abs().mean()) + 1e-9, k  # roundoff grows 4e-7 -> 9e-3 from last to first layer (3 levels of batch-stat BN)


def test_unsup_loss_seven_views_other_lambda_and_pfm():
    """SURVEY 8(f)-1 / A12 beyond the other fixtures: N = 7, odd quarter-resolution size, batch 3, smooth_lambda 0.5; the
    reference's save_pfm / read_pfm against the drop-in's on a random map."""
    import mvs_amd  # noqa: F401
    from mvs_amd.jdacs.datasets import data_io as mine
    g = _fixture("g13_unsup_loss_seven_views")
    gen = torch.Generator().manual_seed(4)
    b, n, h, w = 3, 7, 52, 76
    imgs = F.avg_pool2d(torch.randn(b * n, 3, h, w, generator=gen), 5, 1, 2).view(b, n, 3, h, w) * 3
    K, E = R.synthetic_cameras(n, h // 4, w // 4, w)
    cams = torch.zeros(b, n, 2, 4, 4)
    cams[:, :, 0] = E
    cams[:, :, 1, :3, :3] = K
    db = (600.0 + 40.0 * torch.rand(b, h // 4, w // 4, generator=gen)).requires_grad_(True)
    lb = R.unsup_loss(imgs, cams, db, smooth_lambda=0.5)
    lb.backward()
    la, ga = float(g["loss"]), g["depth_grad"]
    assert abs(la - float(lb)) < 2e-5 * abs(la), (la, float(lb))
    assert float((ga - db.grad).abs().max()) < 2e-6 + 1e-4 * float(ga.abs().max())
    arr = np.random.RandomState(1).rand(17, 23).astype(np.float32) * 900
    assert np.array_equal(arr, g["pfm_array"].numpy())
    ref_bytes = g["pfm_bytes"].numpy().tobytes()
    with tempfile.TemporaryDirectory() as d:
        mine.save_pfm(os.path.join(d, "b.pfm"), arr)
        assert open(os.path.join(d, "b.pfm"), "rb").read() == ref_bytes
        with open(os.path.join(d, "a.pfm"), "wb") as fh:
            fh.write(ref_bytes)
        assert np.array_equal(mine.read_pfm(os.path.join(d, "a.pfm"))[0], g["pfm_read_back"].numpy())
