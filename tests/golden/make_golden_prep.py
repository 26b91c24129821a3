#!/usr/bin/env python3
"""Generate tests/golden/g17_sample_prep.npz by EXECUTING the reference's own functions (build container only).

    python tests/golden/make_golden_prep.py

`jdacs/datasets/dtu_yao.py` and `jdacs-ms/dataset/dtu.py` import cv2 and torchvision at module level and
`jdacs/models/augmentations.py` torchvision: stand-in modules are registered under those names (none of the executed functions
touches them); the trees' argparse configuration is why sys.argv = ["x"].  Executed:
  * center_image of both trees (unbound, self = None) on three seeded 24 x 40 uint8 images and one constant image, and
    jdacs-ms's as written on a 1200 x 1 image (it keeps the first 1184 rows); the 24 x 40 ones once as written (fp32) and
    once on an array whose astype(np.float32) answers float64 -- the same statements evaluated in fp64, the truth the tests
    compare with;
  * RandomGamma.adjust_gamma(clip_image=True) of the three places it is defined, on a 6 x 40 crop in [0, 1], fp32 and fp64;
  * random_image_mask under np.random.seed(SEED) on a [2, 3, 24, 40] tensor with an (8, 13) window.
Only arrays are stored."""
import os
import sys
import types
import warnings

sys.dont_write_bytecode = True
warnings.filterwarnings("ignore")
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sample_prep_oracle as P  # noqa: E402

REF = "/root/reference"
sys.argv = ["x"]
torch.set_num_threads(4)


class _Names(types.ModuleType):
    """every name resolves to `object`: enough for the import and class statements to execute"""
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return object


for name in ("cv2", "torchvision", "torchvision.transforms"):
    sys.modules[name] = _Names(name)
sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]


def tree_modules(tree, names):
    """import `names` with the tree's folder in front of sys.path, then forget its top-level packages so the other tree's
    equally named ones (config, models, ...) can be imported"""
    before = set(sys.modules)
    sys.path.insert(0, os.path.join(REF, tree))
    try:
        mods = [__import__(n, fromlist=["x"]) for n in names]
    finally:
        sys.path.pop(0)
        for k in set(sys.modules) - before:
            if not k.startswith(("PIL", "numpy", "torch", "scipy")):
                del sys.modules[k]
    return mods


dtu_yao, aug = tree_modules("jdacs", ["datasets.dtu_yao", "models.augmentations"])
(dtu_ms,) = tree_modules("jdacs-ms", ["dataset.dtu"])
center = {"jdacs": dtu_yao.MVSDataset.center_image, "jdacs-ms": dtu_ms.DTUDataset.center_image}


class AsF64(np.ndarray):
    """center_image's first statement, img.astype(np.float32), answers float64: the rest of its statements run in fp64"""
    def astype(self, dtype, *a, **k):
        return np.asarray(self, dtype=np.float64)


out = {}
views = P.seeded_views(3, 24, 40, 601)
views = torch.cat([views, torch.full((1, 24, 40, 3), 93, dtype=torch.uint8)], 0)
views[3, :, :, 1] = 255
views[3, :, :, 2] = 0
out["views"] = views.numpy()
c32, c64 = [], []
for m in range(4):
    img = views[m].numpy()
    a, b = center["jdacs"](None, img), center["jdacs-ms"](None, img)
    assert a.dtype == np.float32 and np.array_equal(a, b), "the two trees' center_image disagree"
    c32.append(a)
    t = center["jdacs"](None, img.view(AsF64))
    assert t.dtype == np.float64
    c64.append(np.asarray(t))
    o32, o64 = P.center_image(views[m].float()), P.center_image(views[m].double())
    print("view %d: oracle32 vs reference %.2e, oracle64 vs fp64 run %.2e, reference fp32 vs fp64 %.2e" % (
        m, float((o32 - torch.from_numpy(a)).abs().max()), float((o64 - torch.from_numpy(c64[-1])).abs().max()),
        float(np.abs(a - c64[-1]).max())))
assert np.all(c32[3] == 0) and np.all(c64[3] == 0), "center_image of a constant image is exactly 0"
out["center32"], out["center64"] = np.stack(c32), np.stack(c64)

tall = P.seeded_views(1, 1200, 1, 602)[0]
t32 = center["jdacs-ms"](None, tall.numpy())
assert t32.shape == (1184, 1, 3) and center["jdacs"](None, tall.numpy()).shape == (1200, 1, 3)
out["tall"], out["tall_center32"] = tall.numpy(), t32

crop = views[0, :6].float() / 255
out["gammas"] = np.asarray([0.5, 1.0, 2.0], np.float32)
g32, g64 = [], []
for gamma in out["gammas"].tolist():
    r = [cls.adjust_gamma(crop.clone(), gamma, True) for cls in (aug.RandomGamma, dtu_yao.RandomGamma, dtu_ms.RandomGamma)]
    assert torch.equal(r[0], r[1]) and torch.equal(r[0], r[2])
    g32.append(r[0].numpy())
    g64.append(aug.RandomGamma.adjust_gamma(views[0, :6].double() / 255, gamma, True).numpy())
out["gamma32"], out["gamma64"] = np.stack(g32), np.stack(g64)

SEED = 1234
img = torch.from_numpy(out["center32"][:2]).permute(0, 3, 1, 2).contiguous()
np.random.seed(SEED)
masked, mask = aug.random_image_mask(img, (8, 13))
assert bool((mask == mask[:1, :1]).all())
out["mask_seed"], out["mask_filter_size"] = np.int32(SEED), np.asarray([8, 13], np.int32)
out["mask"] = mask[0, 0].numpy().astype(np.uint8)
out["masked_sum"] = np.float64(masked.double().sum())
assert torch.equal(masked, img * mask)
np.random.seed(SEED)
assert aug.random_image_mask(img, (24, 40))[1] is None

path = os.path.join(HERE, "g17_sample_prep.npz")
np.savez_compressed(path, **out)
print("%s %.1f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))
