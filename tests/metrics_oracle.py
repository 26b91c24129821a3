"""TEST INFRASTRUCTURE: the seven depth-map metrics of the reference's detailed summary (jdacs/train.py:232-238; jdacs/utils.py:
134-163, jdacs/losses/unsup_loss.py:86-125) restated with stock torch ops, in the reference's own op sequence -- a Python loop over
the batch with boolean-mask selections for the four masked metrics, repeat()-ed interval images for the other three.  Used as the
yardstick of ops.depth_metrics (fp32 = the reference's arithmetic, fp64 = the truth the tolerances are derived from) and, on the
GPU, as the stock-op sequence tools/depth_metrics_bench.py times.

Output layout of ops.depth_metrics: out [4+T] = abs error, T threshold rates, mae, less_one, less_three;
per_image [B, 2+T] = abs error and the T rates per image, then the image's term of mae."""
import torch

KEYS = ("abs_depth_error", "thres2mm_error", "thres4mm_error", "thres8mm_error", "mae", "less_one_accuracy", "less_three_accuracy")


def _selected(est, gt, mask, b):
    m = mask[b]
    return est[b][m], gt[b][m]


def abs_depth_error(est, gt, mask):
    """mean |est - gt| over each image's mask, then the mean over the images; also the per-image values"""
    per = []
    for b in range(gt.shape[0]):
        e, g = _selected(est, gt, mask, b)
        per.append(torch.mean((e - g).abs()))
    per = torch.stack(per)
    return per.mean(), per


def thres_rate(est, gt, mask, thres):
    """share of each image's mask pixels with |est - gt| > thres, then the mean over the images; also the per-image values"""
    per = []
    for b in range(gt.shape[0]):
        e, g = _selected(est, gt, mask, b)
        per.append(torch.mean((torch.abs(e - g) > thres).to(est.dtype)))
    per = torch.stack(per)
    return per.mean(), per


def mae_terms(gt, est, interval):
    """per image: (sum |[gt != 0] * (gt - est)| / interval_b) / (count_b + 1e-7); the metric is their SUM"""
    bsz = est.shape[0]
    interval = interval.reshape(bsz)
    nz = torch.ne(gt, 0.0).to(est.dtype)
    denom = torch.sum(nz, dim=[1, 2]) + 1e-7
    total = torch.sum(torch.abs(nz * (gt - est)), dim=[1, 2])
    return (total / interval) / denom


def less_k(gt, est, interval, k):
    """share of the batch's gt != 0 pixels with |gt - est| / interval_b <= k"""
    bsz, h, w = est.shape
    nz = torch.ne(gt, 0.0).to(est.dtype)
    denom = torch.sum(nz) + 1e-7
    interval_image = interval.reshape(bsz, 1, 1).repeat(1, h, w)
    scaled = torch.abs(gt - est) / interval_image
    return torch.sum(nz * torch.le(scaled, k).to(est.dtype)) / denom


def seven(est, gt, mask, interval, thresholds=(2, 4, 8), dtype=torch.float32):
    """(out [4+T], per_image [B,2+T]) in ``dtype``: float32 follows the reference's arithmetic step by step, float64 is the same
    formulas on inputs cast to fp64.  mask: bool, or fp32 (selected where > 0.5).  interval None: NaN for the last three."""
    with torch.no_grad():
        est, gt = est.to(dtype), gt.to(dtype)
        if mask.dtype != torch.bool:
            mask = mask > 0.5
        nan = torch.full((), float("nan"), dtype=dtype, device=est.device)
        a, a_per = abs_depth_error(est, gt, mask)
        rates = [thres_rate(est, gt, mask, t) for t in thresholds]
        if interval is None:
            terms = nan.expand(est.shape[0])
            tail = [nan, nan, nan]
        else:
            interval = interval.to(dtype)
            terms = mae_terms(gt, est, interval)
            tail = [terms.sum(), less_k(gt, est, interval, 1.0), less_k(gt, est, interval, 3.0)]
        out = torch.stack([a] + [r[0] for r in rates] + tail)
        per_image = torch.stack([a_per] + [r[1] for r in rates] + [terms], dim=1)
    return out, per_image


def train_block(est, gt, mask_f32, interval):
    """The block as train.py runs it, scalars read back one by one like tensor2float does: what a validation step costs with the
    stock ops.  Returns the dict of Python floats and the number of .item() reads (the boolean-mask selections synchronise too)."""
    out = {}
    out["abs_depth_error"] = abs_depth_error(est, gt, mask_f32 > 0.5)[0]
    out["thres2mm_error"] = thres_rate(est, gt, mask_f32 > 0.5, 2)[0]
    out["thres4mm_error"] = thres_rate(est, gt, mask_f32 > 0.5, 4)[0]
    out["thres8mm_error"] = thres_rate(est, gt, mask_f32 > 0.5, 8)[0]
    out["mae"] = mae_terms(gt, est, interval).sum()
    out["less_one_accuracy"] = less_k(gt, est, interval, 1.0)
    out["less_three_accuracy"] = less_k(gt, est, interval, 3.0)
    return {k: v.item() for k, v in out.items()}, len(out)


def host_syncs_of_train_block(batch_size):
    """counted from the op sequence above: 4 metrics x B images x 2 boolean-mask selections (a nonzero + size read-back each),
    plus one .item() per scalar"""
    return 4 * batch_size * 2 + len(KEYS)


def seeded_inputs(b, h, w, seed, zero_share=0.3, device="cpu"):
    """est, gt (about ``zero_share`` of it exactly 0), fp32 mask = [gt > 0], intervals: the value ranges of a DTU batch (depths
    425..935 mm, errors of a few mm, intervals about 2.5 mm)"""
    g = torch.Generator().manual_seed(seed)
    gt = 425.0 + 510.0 * torch.rand(b, h, w, generator=g)
    gt = torch.where(torch.rand(b, h, w, generator=g) < zero_share, torch.zeros(()), gt)
    est = gt + 4.0 * torch.randn(b, h, w, generator=g) * torch.rand(b, h, w, generator=g)
    est = torch.where(gt == 0, 425.0 + 510.0 * torch.rand(b, h, w, generator=g), est)
    interval = 2.5 + 0.5 * torch.rand(b, generator=g)
    mask = (gt > 0).float()
    return est.to(device), gt.to(device), mask.to(device), interval.to(device)


def check_against(ours_out, ours_per, ref_out, ref_per, truth_out, truth_per, n_thres, what=""):
    """The acceptance criteria of the metrics, one place for the CPU and the GPU tests (all arguments CPU tensors; ref = the fp32
    reference values, truth = the fp64 ones).  Prints the reference's own error next to ours.
      * NaN-ness equal everywhere;
      * count-based per-image rates and less_*: bit-equal to the fp32 reference (one fp32 division of two exact integers);
      * their means over B <= 8 images: <= 1e-6 relative (at most B - 1 roundings of 2^-24 in another summation order);
      * sum-based values (abs error, mae, per image and for the batch): |ours - truth| <= 1e-6 |truth| (the fp32 per-pixel difference
        contributes <= 2^-24 relative, the sums are fp64 over non-negative terms, at most four fp32 roundings follow), and
        |ours - ref32| <= 1e-6 |ref32| + |ref32 - truth|."""
    T = n_thres
    ours_out, ours_per = ours_out.double(), ours_per.double()
    r_out, r_per, t_out, t_per = ref_out.double(), ref_per.double(), truth_out.double(), truth_per.double()
    assert torch.equal(torch.isnan(ours_out), torch.isnan(r_out)), (what, ours_out, r_out)
    assert torch.equal(torch.isnan(ours_per), torch.isnan(r_per)), (what, ours_per, r_per)
    assert torch.equal(torch.isnan(r_out), torch.isnan(t_out)) and torch.equal(torch.isnan(r_per), torch.isnan(t_per)), what

    def sum_based(o, r, t, name):
        if torch.isnan(t):
            return
        print("%s %s: ours %.9g ref32 %.9g truth %.12g | err ours %.3e ref32 %.3e" % (what, name, o, r, t, abs(o - t), abs(r - t)))
        assert abs(o - t) <= 1e-6 * abs(t), (what, name, float(o), float(t))
        assert abs(o - r) <= 1e-6 * abs(r) + abs(r - t), (what, name, float(o), float(r))

    def count_exact(o, r, t, name):
        if torch.isnan(r):
            return
        print("%s %s: ours %.9g ref32 %.9g truth %.12g | err ours %.3e ref32 %.3e" % (what, name, o, r, t, abs(o - t), abs(r - t)))
        assert float(o) == float(r), (what, name, float(o), float(r))

    def count_mean(o, r, t, name):
        if torch.isnan(r):
            return
        print("%s %s: ours %.9g ref32 %.9g truth %.12g | err ours %.3e ref32 %.3e" % (what, name, o, r, t, abs(o - t), abs(r - t)))
        assert abs(o - r) <= 1e-6 * abs(r), (what, name, float(o), float(r))

    sum_based(ours_out[0], r_out[0], t_out[0], "abs")
    sum_based(ours_out[1 + T], r_out[1 + T], t_out[1 + T], "mae")
    for j in range(T):
        count_mean(ours_out[1 + j], r_out[1 + j], t_out[1 + j], "thres[%d]" % j)
    count_exact(ours_out[2 + T], r_out[2 + T], t_out[2 + T], "less_one")
    count_exact(ours_out[3 + T], r_out[3 + T], t_out[3 + T], "less_three")
    for b in range(ours_per.shape[0]):
        sum_based(ours_per[b, 0], r_per[b, 0], t_per[b, 0], "abs[%d]" % b)
        sum_based(ours_per[b, 1 + T], r_per[b, 1 + T], t_per[b, 1 + T], "mae_term[%d]" % b)
        for j in range(T):
            count_exact(ours_per[b, 1 + j], r_per[b, 1 + j], t_per[b, 1 + j], "thres[%d][%d]" % (j, b))


# ---- the fixture tests/golden/g16_depth_metrics.npz (written by tests/golden/make_golden_metrics.py) -----------------------------
CASES = ("c1_", "c2_", "c3_", "c4_", "c5_", "c6_")
THRESHOLDS = (2, 4, 8)


def decode_case(g, prefix):
    """The inputs of one fixture case as tensors (g: name -> numpy array or tensor).  gt is stored as int16 = 64 gt - 32768
    (multiples of 1/64 mm; -32768 is gt = 0) and the error as float16; est is the fp32 rounding of their exact sum (so est - gt
    is NOT exact in general, while the pixels placed on the decision values -- gt a multiple of 0.25, error 2, 4, 8, 2.5, 7.5 --
    are).  A case may name a ``base`` case (its number) and store only what differs: the mask, or ``nan_at`` (flat pixel indices
    where est is NaN)."""
    src = "c%d_" % int(g[prefix + "base"]) if prefix + "base" in g else prefix
    gt = (torch.as_tensor(g[src + "gt_s"]).double() + 32768.0) / 64.0
    est = (gt + torch.as_tensor(g[src + "err_h"]).double()).float()
    gt = gt.float()
    mask = torch.as_tensor(g[(prefix if prefix + "mask" in g else src) + "mask"]).bool()
    interval = torch.as_tensor(g[src + "interval"]).float()
    if prefix + "nan_at" in g:
        est.view(-1)[torch.as_tensor(g[prefix + "nan_at"]).long()] = float("nan")
    return est, gt, mask, interval


def fixture_results(g, prefix):
    """(out32 [7], per32 [B,5], out64, per64) of a case: the reference's fp32 values and the fp64 truth"""
    return tuple(torch.as_tensor(g[prefix + k]) for k in ("out32", "per32", "out64", "per64"))


def reference_functions(ref_root, tree):
    """(AbsDepthError_metrics, Thres_metrics, non_zero_mean_absolute_diff, less_one_percentage, less_three_percentage) imported
    from ``ref_root``/``tree`` (``jdacs`` or ``jdacs-ms``).  utils.py imports torchvision at module level (for save_images only): an
    empty stand-in is registered for the import; jdacs/losses/unsup_loss.py imports the tree's argparse configuration, hence
    sys.argv = ["x"].  Both trees use the module names ``utils`` and ``losses``; sys.modules, sys.path and sys.argv are put back."""
    import importlib
    import os
    import sys
    import types
    ours = ("utils", "losses", "config", "models", "torchvision")
    saved = {n: m for n, m in sys.modules.items() if n.split(".")[0] in ours}
    argv, nobytecode = sys.argv, sys.dont_write_bytecode
    for n in saved:
        del sys.modules[n]
    tv = types.ModuleType("torchvision")
    tv.utils = types.ModuleType("torchvision.utils")
    sys.modules["torchvision"], sys.modules["torchvision.utils"] = tv, tv.utils
    sys.argv, sys.dont_write_bytecode = ["x"], True
    sys.path.insert(0, os.path.join(ref_root, tree))
    try:
        u = importlib.import_module("utils")
        ul = importlib.import_module("losses.unsup_loss")
    finally:
        sys.path.pop(0)
        sys.argv, sys.dont_write_bytecode = argv, nobytecode
        for n in [n for n in sys.modules if n.split(".")[0] in ours]:
            del sys.modules[n]
        sys.modules.update(saved)
    return u.AbsDepthError_metrics, u.Thres_metrics, ul.non_zero_mean_absolute_diff, ul.less_one_percentage, ul.less_three_percentage


def reference_values(fns, est, gt, mask, interval, thresholds=THRESHOLDS):
    """(out [4+T], per_image [B,2+T]) from the reference's functions: train.py's block on the batch, and on every image alone for
    the per-image values"""
    absd, thres, mae, l1, l3 = fns

    def block(e, g, m, iv):
        return torch.stack([absd(e, g, m)] + [thres(e, g, m, t) for t in thresholds] + [mae(g, e, iv), l1(g, e, iv), l3(g, e, iv)])
    out = block(est, gt, mask, interval)
    n = 2 + len(thresholds)
    per = torch.stack([block(est[b:b + 1], gt[b:b + 1], mask[b:b + 1], interval[b:b + 1])[:n] for b in range(est.shape[0])])
    return out, per


def same_bits(a, c):
    """equal including the positions of NaNs"""
    return torch.equal(torch.isnan(a), torch.isnan(c)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(c))
