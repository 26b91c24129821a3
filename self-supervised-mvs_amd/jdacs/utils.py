"""Caller-side helpers of the path (jdacs/utils.py:36-76, jdacs/eval.py:125-165): recursive
tensor -> numpy conversion, checkpoint loading with the ``module.`` prefix DataParallel leaves, and writing the depth /
confidence maps as PFM files.  Device-agnostic: nothing here hard-codes ``.cuda()``.

The depth-map metrics of the training scripts' detailed summary (jdacs/utils.py:112-163, called at jdacs/train.py:232-238 and
:319-325) under the reference's names -- ``Thres_metrics``, ``AbsDepthError_metrics``, ``compute_metrics_for_each_image``,
``make_nograd_func``, ``DictAverageMeter`` -- each metric one ``ops.depth_metrics`` call (two HIP launches, no host
synchronisation, csrc/depth_metrics_kernels.h) that returns a 0-dim device tensor; ``depth_metrics`` gives all seven values of
that block from ONE call, and ``DepthMetricsMeter`` averages them over the validation set on the device."""
import os

import numpy as np
import torch

from .. import ops
from .datasets.data_io import save_pfm


def _recursive(fn):
    def wrapper(v):
        if isinstance(v, list):
            return [wrapper(x) for x in v]
        if isinstance(v, tuple):
            return tuple(wrapper(x) for x in v)
        if isinstance(v, dict):
            return {k: wrapper(x) for k, x in v.items()}
        return fn(v)
    return wrapper


@_recursive
def tensor2numpy(v):
    if isinstance(v, np.ndarray):
        return v
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().numpy().copy()
    raise NotImplementedError("invalid input type {} for tensor2numpy".format(type(v)))


@_recursive
def tensor2float(v):
    if isinstance(v, float):
        return v
    if isinstance(v, torch.Tensor):
        return v.data.item()
    raise NotImplementedError("invalid input type {} for tensor2float".format(type(v)))


def load_checkpoint(model, ckpt, strict=True):
    """``ckpt``: a path, the reference's ``{'model': state_dict, ...}`` dict (jdacs/train.py:169) or a bare state_dict; keys
    may carry the ``module.`` prefix of nn.DataParallel (jdacs/eval.py:136-137 loads them into a wrapped model)."""
    if isinstance(ckpt, (str, bytes, os.PathLike)):
        ckpt = torch.load(ckpt, map_location="cpu")
    sd = ckpt["model"] if isinstance(ckpt, dict) and "model" in ckpt and isinstance(ckpt["model"], dict) else ckpt
    sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
    return model.load_state_dict(sd, strict=strict)


def write_depth_img(filename, depth):
    """jdacs/eval.py:110-123: the depth map as an 8-bit PNG, grey = (depth - 500) / 2 through PIL's float -> "L" conversion
    (the reference's own two calls; PIL is the reference's dependency for this file too).  Returns 1 like the reference."""
    from PIL import Image
    d = os.path.dirname(filename)
    if d and not os.path.exists(d):
        os.makedirs(d, exist_ok=True)
    Image.fromarray((np.asarray(depth) - 500) / 2).convert("L").save(filename)
    return 1


def save_depth_outputs(outputs, filenames, outdir, depth_png=False):
    """What jdacs/eval.py:150-164 does with a batch of outputs: ``{}/depth_est/{:0>8}.pfm``-style names (``filename`` is
    the dataset's format string with two slots) -> depth_est and confidence PFM files (+ `<depth>.pfm.png` through
    write_depth_img when depth_png, eval.py:165).  Returns the written paths."""
    outputs = tensor2numpy(outputs)
    written = []
    for name, depth, conf in zip(filenames, outputs["depth"], outputs["photometric_confidence"]):
        for kind, arr in (("depth_est", depth), ("confidence", conf)):
            path = os.path.join(outdir, name.format(kind, ".pfm"))
            os.makedirs(os.path.dirname(path), exist_ok=True)
            save_pfm(path, np.ascontiguousarray(arr, dtype=np.float32))
            written.append(path)
            if depth_png and kind == "depth_est":
                write_depth_img(path + ".png", np.ascontiguousarray(arr, dtype=np.float32))
                written.append(path + ".png")
    return written


def make_nograd_func(func):
    """jdacs/utils.py:24-31: ``func`` run under torch.no_grad()"""
    def wrapper(*f_args, **f_kwargs):
        with torch.no_grad():
            return func(*f_args, **f_kwargs)
    return wrapper


def compute_metrics_for_each_image(metric_func):
    """jdacs/utils.py:134-145, for a caller's OWN metric: ``metric_func(est_i, gt_i, mask_i, *args)`` per batch item, then the mean
    of the stacked results.  The metrics of this module do not go through it: the kernel forms the per-image means itself."""
    def wrapper(depth_est, depth_gt, mask, *args):
        results = [metric_func(depth_est[i], depth_gt[i], mask[i], *args) for i in range(depth_gt.shape[0])]
        return torch.stack(results).mean()
    return wrapper


def Thres_metrics(depth_est, depth_gt, mask, thres):
    """jdacs/utils.py:148-155: per image the share of mask pixels with |est - gt| > thres (strict), then the mean over images.
    mask: bool (``mask > 0.5`` as train.py passes it) or the fp32 mask itself.  0-dim device tensor, not read back."""
    assert isinstance(thres, (int, float))
    return ops.depth_metrics(depth_est, depth_gt, mask, None, (thres,))[0][1]


def AbsDepthError_metrics(depth_est, depth_gt, mask):
    """jdacs/utils.py:158-163: per image the mean |est - gt| over the mask, then the mean over images (the "abs-depth L1" of
    BASELINE.md).  Not differentiable, like the reference's (make_nograd_func)."""
    return ops.depth_metrics(depth_est, depth_gt, mask, None, ())[0][0]


METRIC_KEYS = ("abs_depth_error", "thres2mm_error", "thres4mm_error", "thres8mm_error", "mae", "less_one_accuracy",
               "less_three_accuracy")


def depth_metrics(depth_est, depth_gt, mask, depth_interval):
    """The seven scalar_outputs of jdacs/train.py:232-238 (jdacs-ms/train.py:271-277) as a dict of 0-dim device tensors, from one
    launch pair.  mask: train.py's fp32 mask or ``mask > 0.5``."""
    out = ops.depth_metrics(depth_est, depth_gt, mask, depth_interval, (2, 4, 8))[0]
    return {k: out[i] for i, k in enumerate(METRIC_KEYS)}


class DepthMetricsMeter(object):
    """DictAverageMeter for the seven metrics without ``tensor2float``: ``update`` adds the call's values into fp64 sums ON THE
    DEVICE (the finish kernel does it) and never synchronises; ``mean()`` reads the sums back -- the one synchronisation of a
    validation pass -- and returns the keys DictAverageMeter.mean() would."""

    def __init__(self):
        self._buf = None                # float64 [8]: seven sums, then the update count as int64 bits

    def update(self, depth_est, depth_gt, mask, depth_interval):
        n = len(METRIC_KEYS)
        if self._buf is None:
            self._buf = torch.zeros(n + 1, dtype=torch.float64, device=depth_est.device)
        out = ops.depth_metrics(depth_est, depth_gt, mask, depth_interval, (2, 4, 8),
                                meter=(self._buf[:n], self._buf[n:].view(torch.int64)))[0]
        return {k: out[i] for i, k in enumerate(METRIC_KEYS)}

    @property
    def count(self):
        return 0 if self._buf is None else int(self._buf.cpu()[len(METRIC_KEYS):].view(torch.int64))

    def mean(self):
        if self._buf is None:
            raise RuntimeError("DepthMetricsMeter.mean() before any update()")
        host = self._buf.cpu()
        n = len(METRIC_KEYS)
        count = int(host[n:].view(torch.int64))
        return {k: float(host[i]) / count for i, k in enumerate(METRIC_KEYS)}


class DictAverageMeter(object):
    """jdacs/utils.py:112-131: running sums of dicts of Python floats (what ``tensor2float`` returns)."""

    def __init__(self):
        self.data = {}
        self.count = 0

    def update(self, new_input):
        self.count += 1
        for k, v in new_input.items():
            if not isinstance(v, float):
                raise NotImplementedError("invalid data {}: {}".format(k, type(v)))
            self.data[k] = self.data.get(k, 0.0) + v

    def mean(self):
        return {k: v / self.count for k, v in self.data.items()}
