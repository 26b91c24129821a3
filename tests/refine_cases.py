"""RefineNet on HIP (csrc/refine_kernels.h, mvs_refine_fwd / mvs_refine_bwd, ops.RefineNetFn): the cases shared by
tests/test_refine.py (CPU emulation of the kernel sources) and tests/test_gpu_refine.py (the same cases on the device).  Every case
takes the device.

Kernel-level cases: truth is fp64 autograd on the CPU, ATen fp32 on the CPU the yardstick, the bars are conftest's at their default
slack and floors.  Module-level cases: RefineNet(hip_pass=True) and RefineNet(hip_pass=False) on the same weights (seed 0) are both
measured against R.OracleRefineNet in double; the HIP path's error may be at most slack 4 x the stock path's.

ReLU guard.  A pre-ReLU value within rounding of zero has its mask decided by the rounding, and one flipped mask moves a gradient by
O(1 / pixels): a legitimate difference, not an error.  Every module-level case therefore asserts from the fp64 truth that NO
pre-ReLU value of the four blocks lies within 1e-4 of zero (in units of the block's BatchNorm output: gamma = 1, beta = 0 at
initialisation, unit variance).  Nothing is masked or skipped; the input seeds below were searched for on the CPU so that the
assertion holds (about one seed in 400 at 2x16x24 and one in 40 000 at 1x33x41), and the cases re-check it on every run."""
import copy
import json
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import (assert_as_accurate_as_fp32_reference, assert_grads_as_accurate_as_fp32_reference, calibrate_batchnorm,
                      load_golden)
from oracle import ref_torch as R

TAIL = 1024                       # canary elements behind every exactly-sized buffer a kernel writes
EPS = 1e-5
GUARD = 1e-4
ASSEMBLE_SHAPES = ((20, 28), (64, 96), (66, 98), (132, 164))     # 20x28 -> a 5x7 map, smaller than any tile; 66x98: H, W % 4 != 0
TAIL_ROWS = (35, 64, 65, 768, 4097)
MODES = ("train", "frozen", "eval_grad", "eval_nograd")
# (B, h, w) of the quarter-resolution map -> input seed per statistics kind ("batch": train mode; "running": frozen / eval modes,
# whose statistics come from a calibration batch with seed CALIB_SEED); "mixed": the fallback case (conv2's BatchNorm in .eval())
MODULE_SHAPES = ((2, 16, 24), (1, 33, 41))
SEEDS = {}           # filled below: {(B, h, w, kind): seed}
CALIB_SEED = 7


def _dev_lib(dev):
    from mvs_amd import _lib
    lib = _lib.get()
    assert lib.device_type == dev.type, "the library serves %s tensors, the case runs on %s" % (lib.device_type, dev)
    return lib


def _stream(t):
    from mvs_amd import ops
    return ops._stream(t)


def _owned(n, dev, dtype=torch.float32):
    """an output buffer of exactly n elements, NaN-filled, with TAIL canary elements behind it"""
    buf = torch.full((n + TAIL,), float("nan"), dtype=dtype, device=dev)
    buf[n:] = 12345.0
    return buf


def _check_owned(buf, n, what):
    assert bool((buf[n:] == 12345.0).all()), "%s: wrote behind its %d elements" % (what, n)
    assert not bool(torch.isnan(buf[:n]).any()), "%s: left output elements unwritten" % what
    return buf[:n]


def _ulps(a, b):
    """distance in fp32 units in the last place (same-sign finite values)"""
    return (a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs()


# ------------------------------------------------------------------------------------------------------------------------
# input assembly
# ------------------------------------------------------------------------------------------------------------------------
_ASM = {}


def _assemble_inputs(B, H, W):
    key = (B, H, W)
    if key not in _ASM:
        g = torch.Generator().manual_seed(100000 + 1000 * B + 7 * H + W)
        h, w = H // 4, W // 4
        imgs = torch.randn(B, 3, 3, H, W, generator=g)
        depth = 425.0 + 510.0 * torch.rand(B, h, w, generator=g)
        gx0 = torch.randn(B, 4, h, w, generator=g)            # gradient w.r.t. cat(small, depth), NCHW
        gy = torch.randn(B, h, w, generator=g)                # gradient arriving at depth through the residual
        res = {}
        for dt in (torch.float32, torch.float64):
            img = imgs[:, 0].detach().clone().to(dt).requires_grad_(True)
            d = depth.detach().clone().to(dt).requires_grad_(True)
            x0 = torch.cat((F.interpolate(img, scale_factor=0.25, mode="bilinear"), d.unsqueeze(1)), 1)
            ((x0 * gx0.to(dt)).sum() + (d * gy.to(dt)).sum()).backward()
            res[dt] = (x0.detach(), img.grad, d.grad)
        _ASM[key] = dict(imgs=imgs, depth=depth, gx0=gx0, gy=gy, ref32=res[torch.float32], truth=res[torch.float64])
    return _ASM[key]


def assemble_case(dev, B, H, W):
    lib = _dev_lib(dev)
    inp = _assemble_inputs(B, H, W)
    h, w = H // 4, W // 4
    imgs_d = inp["imgs"].to(dev)
    img = imgs_d[:, 0]                                        # a view: batch stride 3 * 3 * H * W, read in place
    assert img.stride(0) == 9 * H * W and not img.is_contiguous() or B == 1
    depth = inp["depth"].to(dev)
    n = B * h * w * 4
    x0 = _owned(n, dev)
    lib.call("mvs_refine_assemble", img.data_ptr(), img.stride(0), depth.data_ptr(), x0.data_ptr(), B, H, W, h, w, _stream(depth))
    ours = _check_owned(x0, n, "refine_assemble").view(B, h, w, 4).permute(0, 3, 1, 2).cpu()
    ref32, truth = inp["ref32"][0], inp["truth"][0]
    if dev.type == "cpu":
        assert torch.equal(ours, ref32), "emulated assembly is not bit-equal to F.interpolate + cat"
    else:
        assert int(_ulps(ours, ref32).max()) <= 1, "assembly more than 1 ulp from F.interpolate + cat"
    assert_as_accurate_as_fp32_reference(ours, ref32, truth, what="refine_assemble %dx%dx%d" % (B, H, W))
    # backward: 0.25 * g on the four pixels of each cell, zero elsewhere (also the rows / columns beyond 4h, 4w); depth: gy + channel 3
    gx0 = inp["gx0"].to(dev).permute(0, 2, 3, 1).contiguous()
    gy = inp["gy"].to(dev)
    ni, nd = B * 3 * H * W, B * h * w
    gimg, gdepth = _owned(ni, dev), _owned(nd, dev)
    lib.call("mvs_refine_assemble_bwd", gx0.data_ptr(), gy.data_ptr(), gimg.data_ptr(), gdepth.data_ptr(), B, H, W, h, w, _stream(gy))
    gi = _check_owned(gimg, ni, "refine_assemble_bwd image").view(B, 3, H, W).cpu()
    gd = _check_owned(gdepth, nd, "refine_assemble_bwd depth").view(B, h, w).cpu()
    assert_as_accurate_as_fp32_reference(gi, inp["ref32"][1], inp["truth"][1], what="refine_assemble_bwd image")
    assert_as_accurate_as_fp32_reference(gd, inp["ref32"][2], inp["truth"][2], what="refine_assemble_bwd depth")
    assert bool((gi[:, :, 4 * h:, :] == 0).all()) and bool((gi[:, :, :, 4 * w:] == 0).all())
    # without an image gradient: depth only
    gdepth2 = _owned(nd, dev)
    lib.call("mvs_refine_assemble_bwd", gx0.data_ptr(), gy.data_ptr(), None, gdepth2.data_ptr(), B, H, W, h, w, _stream(gy))
    assert torch.equal(_check_owned(gdepth2, nd, "refine_assemble_bwd depth only").cpu(), gd.view(-1))


def assemble_refuses_other_depth_sizes_case(dev):
    import pytest
    lib = _dev_lib(dev)
    img = torch.zeros(1, 3, 64, 96, device=dev)
    depth = torch.zeros(1, 17, 24, device=dev)
    x0 = torch.zeros(1 * 17 * 24 * 4, device=dev)
    with pytest.raises(ValueError, match=r"\[1,3,64,96\] image goes with a \[1,16,24\] depth map, got \[1,17,24\]"):
        lib.call("mvs_refine_assemble", img.data_ptr(), img.stride(0), depth.data_ptr(), x0.data_ptr(), 1, 64, 96, 17, 24, _stream(depth))
    from mvs_amd.jdacs.models.mvsnet import RefineNet
    net = RefineNet().to(dev)
    net.hip_pass = True
    with pytest.raises(ValueError, match=r"depth map, got \[1,17,24\]"):
        net(img, depth)


# ------------------------------------------------------------------------------------------------------------------------
# the one-channel tail
# ------------------------------------------------------------------------------------------------------------------------
_TAILS = {}
NSLOTS = 128


def _tail_inputs(rows, frozen):
    """raw with mean ~ 300 and standard deviation ~ 1 (the depth channel dominates the net's activations: a variance formed as a
    difference of large fp32 numbers would be lost); every pre-ReLU value at least 1e-3 from zero"""
    key = (rows, frozen)
    if key in _TAILS:
        return _TAILS[key]
    g = torch.Generator().manual_seed(31 * rows + int(frozen))
    raw = 300.0 + torch.randn(rows, generator=g)
    gamma, beta = 0.5 + torch.rand(1, generator=g), 0.3 * torch.randn(1, generator=g)
    rm, rv = 300.0 + 0.2 * torch.randn(1, generator=g), 0.8 + 0.4 * torch.rand(1, generator=g)
    depth = 425.0 + 510.0 * torch.rand(rows, generator=g)
    dy = torch.randn(rows, generator=g)

    def z64(r):
        return F.batch_norm(r.double().view(1, 1, -1, 1), rm.double().clone(), rv.double().clone(), gamma.double(), beta.double(), not frozen,
                            0.1, EPS).view(-1)
    for _ in range(3):                # push the values near the ReLU's kink away from it (moves the batch statistics a little: repeat)
        z = z64(raw)
        near = z.abs() < 1e-3
        if not bool(near.any()):
            break
        raw = torch.where(near, raw + torch.where(z >= 0, 4e-3, -4e-3).float(), raw)
    assert bool((z64(raw).abs() >= 1e-3).all())
    res = {}
    for dt in (torch.float32, torch.float64):
        r, ga, be = (t.detach().clone().to(dt).requires_grad_(True) for t in (raw, gamma, beta))
        d = depth.detach().clone().to(dt).requires_grad_(True)
        m, v = rm.to(dt).clone(), rv.to(dt).clone()
        y = d + F.relu(F.batch_norm(r.view(1, 1, -1, 1), m, v, ga, be, not frozen, 0.1, EPS).view(-1))
        y.backward(dy.to(dt))
        res[dt] = dict(y=y.detach(), draw=r.grad, dgamma=ga.grad, dbeta=be.grad, ddepth=d.grad, rm=m, rv=v)
    # the statistic rows as the 32 -> 1 convolution's epilogue leaves them: (sum, sum of squares) of disjoint pieces in fp64
    slots = torch.zeros(NSLOTS, 2, dtype=torch.float64)
    for k in range(NSLOTS):
        piece = raw[k::NSLOTS].double()
        slots[k, 0], slots[k, 1] = piece.sum(), (piece * piece).sum()
    out = _TAILS[key] = dict(raw=raw, gamma=gamma, beta=beta, rm=rm, rv=rv, depth=depth, dy=dy, slots=slots, ref32=res[torch.float32],
                             truth=res[torch.float64])
    return out


def _tail_run(dev, lib, inp, rows, frozen):
    from mvs_amd import ops
    raw, depth, dy = (inp[k].to(dev) for k in ("raw", "depth", "dy"))
    gamma, beta = inp["gamma"].to(dev), inp["beta"].to(dev)
    rm, rv = inp["rm"].clone().to(dev), inp["rv"].clone().to(dev)
    y, stats = _owned(rows, dev), _owned(4, dev)
    st = _stream(raw)
    if frozen:
        stats_t = ops.bn_frozen_stats(gamma, beta, rm, rv, EPS)
        stats[:4] = stats_t.view(-1)
        lib.call("mvs_refine_tail_fwd_frozen", raw.data_ptr(), depth.data_ptr(), stats.data_ptr(), beta.data_ptr(), rows, y.data_ptr(), st)
    else:
        slots = inp["slots"].to(dev)
        lib.call("mvs_refine_tail_fwd", raw.data_ptr(), depth.data_ptr(), slots.data_ptr(), NSLOTS, rows, gamma.data_ptr(), beta.data_ptr(),
                 EPS, 0.1, rm.data_ptr(), rv.data_ptr(), stats.data_ptr(), y.data_ptr(), st)
    draw, aff = _owned(rows, dev), _owned(2, dev)
    rec = torch.full((512 + TAIL,), 5.0, dtype=torch.float64, device=dev)
    lib.call("mvs_refine_tail_bwd", dy.data_ptr(), raw.data_ptr(), stats.data_ptr(), beta.data_ptr(), int(frozen), rows, rec.data_ptr(),
             draw.data_ptr(), aff.data_ptr(), aff.data_ptr() + 4, st)
    assert bool((rec[512:] == 5.0).all()), "refine_tail_bwd wrote behind its 512 records"
    y_ = _check_owned(y, rows, "refine_tail y").cpu()
    stats_ = _check_owned(stats, 4, "refine_tail stats").cpu()
    draw_ = _check_owned(draw, rows, "refine_tail_bwd draw").cpu()
    aff_ = _check_owned(aff, 2, "refine_tail_bwd dgamma / dbeta").cpu()
    return dict(y=y_, stats=stats_, draw=draw_, dgamma=aff_[:1], dbeta=aff_[1:], rm=rm.cpu(), rv=rv.cpu())


def tail_case(dev, rows, frozen):
    lib = _dev_lib(dev)
    inp = _tail_inputs(rows, frozen)
    a = _tail_run(dev, lib, inp, rows, frozen)
    b = _tail_run(dev, lib, inp, rows, frozen)
    for k in a:
        assert torch.equal(a[k], b[k]), "refine tail %s differs between two runs (fixed-order reduction)" % k
    ref, tru = inp["ref32"], inp["truth"]
    what = "refine tail rows=%d %s" % (rows, "frozen" if frozen else "batch")
    assert_as_accurate_as_fp32_reference(a["y"], ref["y"], tru["y"], what=what + " y")
    # statistics: mean and invstd against fp64
    if frozen:
        mean64, var64 = inp["rm"].double(), inp["rv"].double()
        assert torch.equal(a["rm"], inp["rm"]) and torch.equal(a["rv"], inp["rv"]), "the frozen tail moved the running statistics"
    else:
        mean64, var64 = inp["raw"].double().mean().view(1), inp["raw"].double().var(unbiased=False).view(1)
        assert_as_accurate_as_fp32_reference(a["rm"], ref["rm"], tru["rm"], what=what + " running_mean")
        assert_as_accurate_as_fp32_reference(a["rv"], ref["rv"], tru["rv"], what=what + " running_var")
    invstd64 = 1.0 / torch.sqrt(var64 + EPS)
    assert abs(float(a["stats"][0]) - float(mean64)) <= 2.0 ** -23 * 300.0 * 1.01, what + " mean"        # one fp32 rounding of ~300
    assert abs(float(a["stats"][1]) / float(invstd64) - 1.0) <= 4e-7, what + " invstd"                   # not 1e-3: the variance survived
    sc = float(a["stats"][1]) * float(inp["gamma"])
    assert abs(float(a["stats"][2]) - sc) <= 1e-6 * abs(sc) and abs(float(a["stats"][3]) - (float(inp["beta"]) - float(a["stats"][0]) * sc)) <= 1e-3
    grads = {k: a[k] for k in ("draw", "dgamma", "dbeta")}
    assert_grads_as_accurate_as_fp32_reference(grads, {k: ref[k] for k in grads}, {k: tru[k] for k in grads}, what=what)
    assert torch.equal(tru["ddepth"].float(), inp["dy"])           # the depth branch's gradient is dy itself (nothing to compute)


_EVAL_TAIL = {}


def eval_tail_case(dev, h, w):
    lib = _dev_lib(dev)
    if (h, w) not in _EVAL_TAIL:
        g = torch.Generator().manual_seed(17 * h + w)
        x = F.relu(torch.randn(1, 32, h, w, generator=g))
        wt, b = 0.1 * torch.randn(1, 32, 3, 3, generator=g), 0.2 * torch.randn(1, generator=g)
        depth = 425.0 + 510.0 * torch.rand(1, h, w, generator=g)
        f = lambda dt: (F.relu(F.conv2d(x.to(dt), wt.to(dt), b.to(dt), padding=1)).squeeze(1) + depth.to(dt))
        _EVAL_TAIL[(h, w)] = (x, wt, b, depth, f(torch.float32), f(torch.float64))
    x, wt, b, depth, ref32, truth = _EVAL_TAIL[(h, w)]
    xd = x.to(dev).permute(0, 2, 3, 1).contiguous()
    wd, bd, dd = wt.to(dev), b.to(dev), depth.to(dev)
    y = _owned(h * w, dev)
    lib.launch_trace()
    lib.call("mvs_refine_tail_eval", xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), dd.data_ptr(), y.data_ptr(), 1, h, w, _stream(xd))
    assert lib.launch_trace() == ["refine_tail eval"]
    ours = _check_owned(y, h * w, "refine_tail_eval").view(1, h, w).cpu()
    assert_as_accurate_as_fp32_reference(ours, ref32, truth, what="refine_tail_eval %dx%d" % (h, w))


# ------------------------------------------------------------------------------------------------------------------------
# module level
# ------------------------------------------------------------------------------------------------------------------------
def module_inputs(B, h, w, seed, pad=0):
    """imgs [B,3,3,H,W] (the net gets imgs[:, 0]), depth [B,h,w] in 425..935, the weights of the scalar the backward starts from"""
    g = torch.Generator().manual_seed(seed)
    H, W = 4 * h + pad, 4 * w + pad
    imgs = torch.randn(B, 3, 3, H, W, generator=g)
    depth = 425.0 + 510.0 * torch.rand(B, h, w, generator=g)
    gout = torch.randn(B, h, w, generator=g)
    return imgs, depth, gout


def oracle_with_seed0_weights(kind, B, h, w):
    """R.OracleRefineNet in double with the weights RefineNet() gets from seed 0; kind "running" / "mixed": running statistics
    calibrated on another batch (seed CALIB_SEED), so that they differ from the batch statistics of the case's input"""
    from mvs_amd.jdacs.models.mvsnet import RefineNet
    torch.manual_seed(0)
    net = RefineNet()
    ora = R.OracleRefineNet()
    ora.load_state_dict(net.state_dict())
    ora = ora.double()
    if kind != "batch":
        imgs, depth, _ = module_inputs(B, h, w, CALIB_SEED)
        calibrate_batchnorm(ora, imgs[:, 0].double(), depth.double())
    return ora.train()


def set_mode(net, mode):
    """train: batch statistics; frozen: the idiom (net.train(), every BatchNorm in .eval()); eval_*: net.eval(); mixed: conv2's
    BatchNorm alone in .eval()"""
    net.train()
    if mode in ("eval_grad", "eval_nograd"):
        net.eval()
    elif mode == "frozen":
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eval()
    elif mode == "mixed":
        net.conv2.bn.eval()
    return net


def relu_guard(ora, img, depth):
    """-> the number of pre-ReLU values of the four blocks within GUARD of zero in the fp64 oracle (state and mode as they are)"""
    seen = []
    hooks = [getattr(ora, n).bn.register_forward_hook(lambda m, i, o: seen.append(o.detach())) for n in ("conv1", "conv2", "conv3", "res")]
    try:
        state = copy.deepcopy(ora.state_dict())
        with torch.no_grad():
            ora(img, depth)
        ora.load_state_dict(state)            # (a train-mode forward moved the running statistics)
    finally:
        for hk in hooks:
            hk.remove()
    assert len(seen) == 4
    return sum(int((z.abs() < GUARD).sum()) for z in seen)


def _leaves(imgs, depth, dev, dtype=torch.float32):
    imgs = imgs.detach().clone().to(device=dev, dtype=dtype).requires_grad_(True)     # the leaf is the 5-D tensor; the net reads the view imgs[:, 0]
    d = depth.detach().clone().to(device=dev, dtype=dtype).requires_grad_(True)
    return imgs, d


def _module_triple(dev, mode, B, h, w, kind, pad=0):
    """(hip, stock, truth) results of one case; asserts the ReLU guard on the truth first"""
    from mvs_amd.jdacs.models.mvsnet import RefineNet
    seed = SEEDS[(B, h, w, kind)]
    imgs, depth, gout = module_inputs(B, h, w, seed, pad)
    ora = set_mode(oracle_with_seed0_weights(kind, B, h, w), mode)
    near = relu_guard(ora, imgs[:, 0].double(), depth.double())
    assert near == 0, "seed %d: %d pre-ReLU values of the fp64 truth within %g of zero (%s, %dx%dx%d)" % (seed, near, GUARD, mode, B, h, w)
    grad = mode != "eval_nograd"
    results = []
    for hip in (True, False, None):
        if hip is None:
            net, dt, d = copy.deepcopy(ora), torch.float64, torch.device("cpu")
        else:
            net = RefineNet()
            net.load_state_dict({k: v.float() for k, v in ora.state_dict().items()})
            net.hip_pass = hip
            net, dt, d = set_mode(net.to(dev), mode), torch.float32, dev
        im, dp = _leaves(imgs, depth, d, dt)
        net.zero_grad(set_to_none=True)
        res = {}
        if grad:
            out = net(im[:, 0], dp)
            (out * gout.to(device=d, dtype=dt)).sum().backward()
            res["grads"] = {k: p.grad.detach().cpu() for k, p in net.named_parameters()}
            res["grads"]["depth"] = dp.grad.detach().cpu()
            res["grads"]["image"] = im.grad[:, 0].detach().cpu()
            assert bool((im.grad[:, 1:] == 0).all())
        else:
            with torch.no_grad():
                out = net(im[:, 0], dp)
        res["out"] = out.detach().cpu()
        sd = net.state_dict()
        res["running"] = {k: sd[k].detach().cpu().clone() for k in sorted(sd) if "running" in k}
        res["counters"] = [int(sd[k]) for k in sorted(sd) if "num_batches" in k]
        results.append(res)
    return results


def _compare(hip, stock, truth, what, grad):
    assert_as_accurate_as_fp32_reference(hip["out"], stock["out"], truth["out"], what=what + " refined depth")
    assert hip["counters"] == stock["counters"] == truth["counters"], what + " num_batches_tracked"
    # (per buffer and relative, the criterion of the gradients: conv1's running_var is ~1e4 -- the depth channel -- and the last
    #  block's ~1e-2, so one absolute bar over all of them would only look at the largest)
    assert_grads_as_accurate_as_fp32_reference(hip["running"], stock["running"], truth["running"], what=what + " running statistics")
    if grad:
        assert set(hip["grads"]) == set(truth["grads"])
        assert_grads_as_accurate_as_fp32_reference(hip["grads"], stock["grads"], truth["grads"], what=what)


def modes_case(dev, mode, B, h, w):
    from mvs_amd import ops
    lib = _dev_lib(dev)
    kind = "batch" if mode == "train" else "running"
    lib.launch_trace()
    hip, stock, truth = _module_triple(dev, mode, B, h, w, kind)
    what = "RefineNet %s %dx%dx%d" % (mode, B, h, w)
    _compare(hip, stock, truth, what, mode != "eval_nograd")
    if mode == "train":
        assert hip["counters"] == [1, 1, 1, 1]
    else:
        assert hip["counters"] == [1, 1, 1, 1], what            # (the calibration batch's; this call counted nothing)
        for k, v in truth["running"].items():
            assert torch.equal(hip["running"][k], v.float()), "%s: %s moved" % (what, k)
    assert hasattr(ops, "RefineNetFn")


def fallback_case(dev):
    """one BatchNorm in .eval(), the rest training: the per-block path, exactly as with hip_pass off"""
    from mvs_amd.jdacs.models.mvsnet import RefineNet
    lib = _dev_lib(dev)
    B, h, w = MODULE_SHAPES[0]
    torch.manual_seed(0)
    probe = set_mode(RefineNet().to(dev), "mixed")
    probe.hip_pass = True
    imgs, depth, _ = module_inputs(B, h, w, SEEDS[(B, h, w, "mixed")])
    assert probe.hip_pass_mode(imgs[:, 0].to(dev), depth.to(dev)) is None
    assert set_mode(probe, "train").hip_pass_mode(imgs[:, 0].to(dev), depth.to(dev)) == "train"
    assert probe.hip_pass_mode(imgs[:, 0].to(dev).double(), depth.to(dev).double()) is None          # not fp32
    probe.conv3.bn.momentum = None
    assert probe.hip_pass_mode(imgs[:, 0].to(dev), depth.to(dev)) is None                            # cumulative average
    lib.launch_trace()
    hip, stock, truth = _module_triple(dev, "mixed", B, h, w, "mixed")
    assert not any(lab.startswith("refine_") for lab in lib.launch_trace())
    assert torch.equal(hip["out"], stock["out"]) and all(torch.equal(hip["running"][k], v) for k, v in stock["running"].items())
    if dev.type == "cpu":          # (on the GPU the per-block path's own backward differs between two runs: the library's weight gradients,
        for k, v in stock["grads"].items():       # the order of the fp64 slot atomics -- there the bar below is the comparison)
            assert torch.equal(hip["grads"][k], v), k
    _compare(hip, stock, truth, "RefineNet with one frozen BatchNorm", True)


TRAIN_LABELS = ["refine_assemble", "refine_tail", "refine_tail_bwd_reduce", "refine_tail_bwd", "refine_assemble_bwd"]


def launch_trace_case(dev):
    """what a call launches, by label (mvs_launch_trace; an input gradient's pack + pass share one label): train 10 forward + 19
    backward, frozen with "refine_tail frozen", eval 5"""
    from mvs_amd.jdacs.models.mvsnet import RefineNet
    lib = _dev_lib(dev)
    B, h, w = 1, 8, 12
    imgs, depth, gout = module_inputs(B, h, w, 1)
    torch.manual_seed(0)
    net = RefineNet().to(dev)
    net.hip_pass = True
    traces = {}
    for mode in ("train", "frozen", "eval_nograd"):
        set_mode(net, mode)
        for _ in range(2):                                 # the second call: the folded weight images of eval mode are cached
            im, dp = _leaves(imgs, depth, dev)
            lib.launch_trace()
            if mode == "eval_nograd":
                with torch.no_grad():
                    net(im[:, 0], dp)
                traces[mode] = lib.launch_trace()
                continue
            # the trace is per thread, and on the GPU the backward pass runs on autograd's device thread: cleared there when the
            # node's output gradient arrives, read there when its depth gradient leaves
            out = net(im[:, 0], dp)
            fwd, bwd = lib.launch_trace(), []
            out.register_hook(lambda g_: (lib.launch_trace(), None)[1])
            dp.register_hook(lambda g_, bwd=bwd: (bwd.extend(lib.launch_trace()), None)[1])
            (out * gout.to(dev)).sum().backward()
            traces[mode] = fwd + bwd
    t = traces["train"]
    assert [lab for lab in t if lab.startswith("refine_")] == TRAIN_LABELS, t
    assert t[0] == "refine_assemble" and t[1] == "conv2d_pack_weights_batch" and t[9] == "refine_tail" and t[-1] == "refine_assemble_bwd", t
    assert len(t) == 29 and sum(lab.startswith("conv2d_igemm") for lab in t[:10]) == 4, t
    f = traces["frozen"]
    assert [lab for lab in f if lab.startswith("refine_")] == ["refine_assemble", "refine_tail frozen"] + TRAIN_LABELS[2:], f
    assert f.count("bn_frozen_stats") == 4 and not any(lab in ("bn_relu_fwd_slots", "bn_finalize_slots", "bn_relu_bwd_slots") for lab in f), f
    e = traces["eval_nograd"]
    assert len(e) == 5 and e[0] == "refine_assemble" and e[4] == "refine_tail eval" and all(lab.startswith("conv2d_igemm") for lab in e[1:4]), e
    return net, imgs, depth, gout


_OURS = ("conv2d_", "bn_", "refine_", "void conv2d_", "void bn_", "void refine_")


def no_library_kernel_case(dev):
    """GPU only: the device kernels of one train step of the refine net under torch.profiler -- no MIOpen kernel, no ATen convolution
    or batch-norm kernel (ATen's fill / elementwise kernels of the surrounding test code are not the net's)"""
    import re
    from torch.profiler import ProfilerActivity, profile
    net, imgs, depth, gout = launch_trace_case(dev)
    set_mode(net, "train")
    go = gout.to(dev)

    def step():
        im, dp = _leaves(imgs, depth, dev)
        (net(im[:, 0], dp) * go).sum().backward()
    step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        step()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]
    assert sum(n.startswith(_OURS) for n in names) >= 30, names
    bad = [n for n in names if not n.startswith(_OURS) and re.search(r"miopen|conv|batch_?norm|gemm|winograd|Cijk|ck::", n, re.I)]
    assert not bad, "library kernels in the refine step: %r" % bad


# ------------------------------------------------------------------------------------------------------------------------
# MVSNet(refine=True) against the reference's fixture
# ------------------------------------------------------------------------------------------------------------------------
def _fixture():
    out = {}
    for part in "abc":
        out.update(load_golden("g13_mvsnet_five_views_" + part))
    return out


def _err(a, ref):
    ref = ref.double()
    return float((a.double().cpu() - ref).abs().sum()) / (float(ref.abs().sum()) + 1e-300)


def fixture_case(dev):
    """tests/test_oracle_vs_reference.py:47-66 on the device.  The bound is not fixed in advance: the HIP model's error against the
    fixture may be at most 4 x the error of R.OracleMVSNet(refine=True) run with stock ops on the same device, plus conftest's floors
    (2e-6 forward, 2e-5 gradients, relative L1).  Both numbers per tensor are appended to refine_parity_ratios.jsonl (the copy kept
    with the project: profiles/refine_parity_ratios.jsonl; measured worst ratio 1.31).  The seeds are the fixture's, so the ReLU guard
    cannot be chosen here: its count on the fp64 oracle (7 of 74 k values) is printed and recorded, and the bound -- relative to the
    oracle's own error on the same device, which meets the same seven values -- is what covers them."""
    from mvs_amd.jdacs.models.mvsnet import MVSNet, RefineNet
    g = _fixture()
    torch.manual_seed(0)
    ora = R.OracleMVSNet(refine=True)
    with torch.no_grad():
        ora.cost_regularization.prob.weight.mul_(50.0)
    for k, v in ora.state_dict().items():
        assert float(v.double().sum()) == float(g["sdsum." + k]), k
    imgs, proj, dv = R.synthetic_mvsnet_inputs(2, 5, 64, 96, 16, seed=3)
    net = MVSNet(refine=True)
    net.load_state_dict(ora.state_dict())
    net.refine_network.hip_pass = True
    res = {}
    for name, model in (("hip", net.to(dev)), ("oracle", copy.deepcopy(ora).to(dev))):
        r = res[name] = {}
        for mode in ("train", "eval"):
            getattr(model, mode)()
            model.zero_grad(set_to_none=True)
            if mode == "train":
                b = model(imgs.to(dev), proj.to(dev), dv.to(dev))
                b["depth"].mean().backward()
                for k, q in model.named_parameters():
                    if q.grad is not None and not k.endswith("prob.bias"):
                        r["grad." + k] = q.grad.detach().cpu()
            else:
                with torch.no_grad():
                    b = model(imgs.to(dev), proj.to(dev), dv.to(dev))
            r[mode + "_depth"], r[mode + "_conf"] = b["depth"].detach().cpu(), b["photometric_confidence"].detach().cpu()
    keys = sorted(res["hip"])
    assert set(keys) == set(res["oracle"]) and any(k.startswith("grad.refine_network.res.bn") for k in keys)
    assert all(k in g for k in keys)
    # the ReLU guard's count, for the record: the refine net of the fp64 oracle on the CPU, train mode, on the oracle's own depth
    o64 = copy.deepcopy(ora).double().train()
    o64.refine = False
    with torch.no_grad():
        d64 = o64(imgs.double(), proj.double(), dv.double())["depth"]
    near = relu_guard(o64.refine_network, imgs[:, 0].double(), d64)
    print("pre-ReLU values of the refine net within %g of zero (fp64 oracle): %d" % (GUARD, near))
    rows, bad = [], []
    for k in keys:
        e_h, e_o = _err(res["hip"][k], g[k]), _err(res["oracle"][k], g[k])
        floor = 2e-5 if k.startswith("grad.") else 2e-6
        rows.append({"tensor": k, "hip_err": e_h, "oracle_err": e_o, "ratio": e_h / max(e_o, 1e-300), "slack_allowed": 4.0, "floor": floor})
        print("%-50s hip %.3e oracle %.3e" % (k, e_h, e_o))
        if e_h > 4.0 * e_o + floor:
            bad.append("%s: HIP %.3e vs oracle-on-device %.3e" % (k, e_h, e_o))
    # written next to the file MVS_GRAD_REPORT names, like tests/conv2d_arm_cases.py's report (nowhere when it is unset: a test run
    # leaves the checkout as it was); the copy kept with the project is profiles/refine_parity_ratios.jsonl
    out_dir = os.path.dirname(os.path.abspath(os.environ["MVS_GRAD_REPORT"])) if os.environ.get("MVS_GRAD_REPORT") else ""
    if out_dir:
        try:
            with open(os.path.join(out_dir, "refine_parity_ratios.jsonl"), "a") as fh:
                for row in rows:
                    fh.write(json.dumps(dict(row, what="MVSNet(refine=True) vs g13_mvsnet_five_views", device=str(dev),
                                             relu_guard_count=near)) + "\n")
        except OSError:
            pass
    assert not bad, "less accurate than the oracle on the same device: " + "; ".join(bad)
    assert isinstance(net.refine_network, RefineNet)


# the searched input seeds (`python tests/refine_cases.py search` repeats the search on the CPU)
SEEDS.update({(2, 16, 24, "batch"): 244, (2, 16, 24, "running"): 1748, (2, 16, 24, "mixed"): 425, (1, 33, 41, "running"): 21168,
              (1, 33, 41, "batch"): 58917})


def _search(B, h, w, kind, start=0, stop=10 ** 7):
    mode = {"batch": "train", "running": "frozen", "mixed": "mixed"}[kind]
    ora = set_mode(oracle_with_seed0_weights(kind, B, h, w), mode)
    for seed in range(start, stop):
        imgs, depth, _ = module_inputs(B, h, w, seed)
        if relu_guard(ora, imgs[:, 0].double(), depth.double()) == 0:
            return seed
    return None


if __name__ == "__main__":
    import sys
    torch.set_num_threads(1)
    if sys.argv[1:2] == ["search"]:
        todo = [(b, h, w, k) for (b, h, w) in MODULE_SHAPES for k in ("batch", "running")] + [MODULE_SHAPES[0] + ("mixed",)]
        if len(sys.argv) > 2:
            todo = [todo[int(sys.argv[2])]]
        for b, h, w, k in todo:
            print((b, h, w, k), _search(b, h, w, k), flush=True)
