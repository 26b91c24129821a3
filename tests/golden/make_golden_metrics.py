#!/usr/bin/env python3
"""Generate tests/golden/g16_depth_metrics.npz by IMPORTING the reference's metric functions (build container only).

    python tests/golden/make_golden_metrics.py

`utils.py` of both trees imports torchvision at module level (for save_images only); an empty stand-in module is registered under
that name, and `jdacs/losses/unsup_loss.py` imports the tree's argparse configuration, hence sys.argv = ["x"] -- both inside
tests/metrics_oracle.py:reference_functions, which the live comparison of tests/test_depth_metrics.py uses too.  Only arrays are stored:
the seeded inputs (tests/metrics_oracle.py:decode_case says how), the seven fp32 values and the per-image values the reference
returns, and the same formulas evaluated on inputs cast to fp64 by tests/metrics_oracle.py -- whose fp32 evaluation is asserted to
reproduce the reference bit for bit here.  The functions of jdacs-ms are asserted to return the same bits as those of jdacs."""
import os
import sys
import warnings

sys.dont_write_bytecode = True
warnings.filterwarnings("ignore")
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import metrics_oracle as M  # noqa: E402

REF = "/root/reference"
torch.set_num_threads(4)
TREES = {t: M.reference_functions(REF, t) for t in ("jdacs", "jdacs-ms")}


def quantised_inputs(b, h, w, seed, zero_share=0.3):
    g = torch.Generator().manual_seed(seed)
    gt_q = torch.randint(425 * 64, 935 * 64, (b, h, w), generator=g)
    gt_q = torch.where(torch.rand(b, h, w, generator=g) < zero_share, torch.zeros((), dtype=torch.long), gt_q)
    err = (4.0 * torch.randn(b, h, w, generator=g) * torch.rand(b, h, w, generator=g)).half()
    return gt_q, err


def finish(out, prefix, arrays):
    est, gt, mask, interval = M.decode_case(arrays, prefix)
    r_out, r_per = M.reference_values(TREES["jdacs"], est, gt, mask, interval)
    m_out, m_per = M.reference_values(TREES["jdacs-ms"], est, gt, mask, interval)
    same = M.same_bits
    assert same(r_out, m_out) and same(r_per, m_per), "jdacs and jdacs-ms disagree"
    o32, p32 = M.seven(est, gt, mask, interval, M.THRESHOLDS, torch.float32)
    assert same(o32, r_out) and same(p32, r_per), "the restated formulas do not reproduce the reference bit for bit: " + prefix
    o64, p64 = M.seven(est, gt, mask, interval, M.THRESHOLDS, torch.float64)
    arrays.update({prefix + "out32": r_out.numpy(), prefix + "per32": r_per.numpy(), prefix + "out64": o64.numpy(),
                   prefix + "per64": p64.numpy()})
    out.update({k: v for k, v in arrays.items() if k.startswith(prefix)})
    print("%s B=%d %dx%d mask %d of %d | %s" % (prefix, est.shape[0], est.shape[1], est.shape[2], int(mask.sum()), mask.numel(),
                                               " ".join("%.6g" % v for v in r_out.tolist())))
    print("   fp32-vs-fp64 relative: %s" % " ".join("%.1e" % v for v in ((r_out.double() - o64).abs() / o64.abs()).tolist()))


def case1_arrays():
    gt_q, err = quantised_inputs(3, 37, 53, 161)
    # eight pixels of the image with interval 2.5 sit exactly on a decision value: |e| = 2, 4, 8 (both signs: six pixels) and
    # |e| / 2.5 = 1, 3; their gt is a multiple of 0.25, so est = gt + e and est - gt are exact in fp32
    on_value = [2.0, -2.0, 4.0, -4.0, 8.0, -8.0, 2.5, -7.5]
    for i, e in enumerate(on_value):
        y, x = 3 + 4 * i, 5 + 5 * i
        gt_q[1, y, x] = (500 + 37 * i) * 64 + 16 * (i % 4)
        err[1, y, x] = e
    return {"c1_gt_s": (gt_q - 32768).numpy().astype(np.int16), "c1_err_h": err.numpy(), "c1_mask": (gt_q > 0).numpy().astype(np.uint8),
            "c1_interval": np.asarray([2.65, 2.5, 3.0], np.float32)}, len(on_value)


out = {}
arrays, n_on = case1_arrays()
est, gt, mask, interval = M.decode_case(arrays, "c1_")
d = (est - gt).abs()[1]
assert int(((d == 2) | (d == 4) | (d == 8)).sum()) >= 6 and int(((d / 2.5 == 1) | (d / 2.5 == 3)).sum()) >= 2
assert 0.25 < float((gt == 0).float().mean()) < 0.35
finish(out, "c1_", arrays)

gt_q, err = quantised_inputs(2, 67, 131, 162)            # 8777 pixels per image: two whole 4096-pixel tiles and a ragged third
arrays.update({"c2_gt_s": (gt_q - 32768).numpy().astype(np.int16), "c2_err_h": err.numpy(), "c2_mask": (gt_q > 0).numpy().astype(np.uint8),
               "c2_interval": np.asarray([2.5, 2.8], np.float32)})
finish(out, "c2_", arrays)

m3 = arrays["c1_mask"].copy()
m3[2] = 0                                                # one image's mask empty: NaN for its values and the batch means
arrays.update({"c3_base": np.int32(1), "c3_mask": m3})
finish(out, "c3_", arrays)

flat_mask = torch.from_numpy(arrays["c1_mask"]).view(-1)
on_idx, off_idx = torch.nonzero(flat_mask)[:, 0], torch.nonzero(flat_mask == 0)[:, 0]
arrays.update({"c4_base": np.int32(1), "c4_nan_at": np.asarray([int(on_idx[777])], np.int64)})      # NaN in est at a mask pixel
finish(out, "c4_", arrays)
arrays.update({"c5_base": np.int32(1), "c5_nan_at": np.asarray([int(off_idx[333])], np.int64)})     # NaN at a gt == 0 pixel
finish(out, "c5_", arrays)
assert bool(torch.isnan(torch.from_numpy(out["c5_out32"])).tolist() == [False] * 4 + [True] + [False] * 2)

gt_q, err = quantised_inputs(2, 29, 41, 166)
rnd = (torch.rand(2, 29, 41, generator=torch.Generator().manual_seed(167)) < 0.5)
assert int((rnd != (gt_q > 0)).sum()) > 500              # a mask that is NOT [gt != 0]
arrays.update({"c6_gt_s": (gt_q - 32768).numpy().astype(np.int16), "c6_err_h": err.numpy(), "c6_mask": rnd.numpy().astype(np.uint8),
               "c6_interval": np.asarray([2.5, 3.1], np.float32)})
finish(out, "c6_", arrays)

path = os.path.join(HERE, "g16_depth_metrics.npz")
np.savez_compressed(path, **out)
print("%s %.1f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))
