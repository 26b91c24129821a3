"""Frozen-statistics BatchNorm (bn.training == False, autograd on): the cases shared by tests/test_frozen_bn.py (CPU emulation of the
kernel sources) and tests/test_gpu_frozen_bn.py (the same cases, same shapes, on the device).  Every case takes the device.

Arithmetic under test, per channel: scale = gamma/sqrt(running_var+eps), shift = beta - running_mean*scale, z = raw*scale + shift,
y = relu?(z) (+ skip), dyh = dy*[z > 0], draw = scale*dyh, dbeta = sum dyh, dgamma = sum dyh*(raw - running_mean)*invstd; the
running statistics and num_batches_tracked are never written."""
import copy
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import GOLDEN, assert_grads_as_accurate_as_fp32_reference, load_golden, rel_l1, state_dict_from
from oracle import ref_torch as R

CL3 = torch.channels_last_3d
EPS = 1e-5
KERNEL_CHANNELS = (4, 8, 16, 32, 64)
KERNEL_DIMS = {105: (3, 5, 7), 4096: (16, 16, 16)}    # 105 rows: n4 below one workgroup at C = 4 and no multiple of 256
_BN = nn.modules.batchnorm._BatchNorm


def load_parts(name):
    """a fixture written as <name>.npz, <name>_b.npz, ... with disjoint keys (tests/golden/make_golden_frozen_bn.py)"""
    out = load_golden(name)
    for suffix in "bcdefgh":
        if not os.path.exists(os.path.join(GOLDEN, "%s_%s.npz" % (name, suffix))):
            break
        out.update(load_golden("%s_%s" % (name, suffix)))
    return out


def freeze_batchnorm(net):
    """the usual idiom: the model trains, every BatchNorm module is in .eval()"""
    net.train()
    for m in net.modules():
        if isinstance(m, _BN):
            m.eval()
    return net


def leaf(t, dev, fmt=None):
    """a fresh leaf on the device (Tensor.to() returns the tensor itself when nothing changes, and .grad would accumulate on it)"""
    t = t.detach().clone().to(dev)
    if fmt is not None:
        t = t.contiguous(memory_format=fmt)
    return t.requires_grad_(True)


def buffers_of(net):
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items() if "running" in k or "num_batches" in k}


def assert_buffers_untouched(before, net, what=""):
    after = buffers_of(net)
    for k, v in before.items():
        assert torch.equal(v, after[k]), "%s: %s changed" % (what, k)


# ------------------------------------------------------------------------------------------------------------------------
# kernels vs fp64 autograd
# ------------------------------------------------------------------------------------------------------------------------
_KERNEL_INPUTS = {}


def kernel_inputs(C, rows):
    """Seeded CPU inputs, shared by every case of one (C, rows).  Channel 1 has gamma = 0 (draw = 0, dgamma from xhat alone),
    channel 2 is negative everywhere (mask closed: all-zero row sums), channel 3 has running_mean = beta = 0 and a handful of raw
    values exactly 0, so z == 0 exactly (mask closed, as `>` says).  Everywhere else |z| >= 1e-3: the mask of a value within fp32
    rounding of zero would be decided by the rounding (fused or not, fp32 or fp64), not by the kernel."""
    key = (C, rows)
    if key in _KERNEL_INPUTS:
        return _KERNEL_INPUTS[key]
    g = torch.Generator().manual_seed(1000 * C + rows)
    shape = (1, C) + KERNEL_DIMS[rows]
    raw = torch.randn(shape, generator=g)
    rm, rv = torch.randn(C, generator=g) * 0.5, 0.5 + torch.rand(C, generator=g)
    gamma, beta = 0.5 + torch.rand(C, generator=g), torch.randn(C, generator=g) * 0.3
    gamma[1] = 0.0
    beta[2] = -50.0
    rm[3], beta[3] = 0.0, 0.0
    v = lambda t: t.view(1, C, 1, 1, 1)
    sc = gamma / torch.sqrt(rv + EPS)
    sh = beta - rm * sc
    z = raw.double() * v(sc).double() + v(sh).double()
    near = (z.abs() < 1e-3) & (v(sc) != 0)
    raw = torch.where(near, raw + torch.where(z >= 0, 1.0, -1.0).float() * 2e-3 / v(sc).clamp_min(1e-3), raw)
    raw[0, 3].view(-1)[::7] = 0.0
    raw[0, 3].view(-1)[3] = -0.0
    z = raw.double() * v(sc).double() + v(sh).double()
    assert bool(((z.abs() >= 1e-3) | (z == 0) | (v(sc) == 0)).all()) and bool((z[0, 2] < 0).all()) and int((z[0, 3] == 0).sum()) >= 15
    dy = torch.randn(shape, generator=g)
    skip = torch.randn(shape, generator=g)
    gy8 = torch.randn((1, 8) + KERNEL_DIMS[rows], generator=g)
    w8 = torch.randn((8, C, 3, 3, 3), generator=g) * 0.2
    out = _KERNEL_INPUTS[key] = dict(raw=raw, rm=rm, rv=rv, gamma=gamma, beta=beta, dy=dy, skip=skip, gy8=gy8, w8=w8)
    return out


def _truth64(inp, dy, relu, with_skip):
    """fp64 autograd of relu?(batch_norm(raw, rm, rv, gamma, beta, training=False)) (+ skip)"""
    raw, gamma, beta = (inp[k].double().requires_grad_(True) for k in ("raw", "gamma", "beta"))
    skip = inp["skip"].double().requires_grad_(True)
    y = F.batch_norm(raw, inp["rm"].double(), inp["rv"].double(), gamma, beta, False, 0.0, EPS)
    if relu:
        y = F.relu(y)
    if with_skip:
        y = y + skip
    y.backward(dy.double())
    return y.detach(), raw.grad, gamma.grad, beta.grad, (skip.grad if with_skip else None)


_PREFILLED = {}


def _prefilled(inp, C, rows, relu, dev, stats, raw_d):
    """(dy, slots): an output gradient written by an input-gradient kernel whose bn_raw epilogue was handed the FROZEN stats --
    ops.conv3d_dgrad(bn=...) of an 8-channel consumer.  That epilogue always applies the ReLU mask (the blocks it serves have
    one), so relu = 0 takes the other producer of the same sums, mvs_bn_bwd_reduce_slots(relu=0), on dy = inp['dy'].
    Computed once per (C, rows, relu, device): the slots are only read by the pass under test."""
    from mvs_amd import ops
    key = (C, rows, relu, str(dev))
    if key not in _PREFILLED:
        lib = ops._lib_for(raw_d)
        (slots,) = ops.stat_slots(raw_d, 1, ops.bn_nslots(lib, C), C, 1)
        if relu:
            dy = ops.conv3d_dgrad(inp["gy8"].to(dev), inp["w8"].to(dev), tuple(raw_d.shape), 1, False, bn=(raw_d, stats, slots))
        else:
            dy = inp["dy"].to(dev).contiguous(memory_format=CL3)
            lib.call("mvs_bn_bwd_reduce_slots", ops._p(dy), ops._p(raw_d), ops._p(stats), int(relu), 1, raw_d.numel() // C, C,
                     ops._p(slots), slots.shape[-3], ops._stream(raw_d))
        _PREFILLED[key] = (dy, slots)
    return _PREFILLED[key]


def kernel_case(dev, C, rows, relu, with_skip, form):
    from mvs_amd import ops
    inp = kernel_inputs(C, rows)
    raw_d = inp["raw"].to(dev).contiguous(memory_format=CL3)
    p = {k: inp[k].to(dev) for k in ("rm", "rv", "gamma", "beta")}
    lib = ops._lib_for(raw_d)
    stats = ops.bn_frozen_stats(p["gamma"], p["beta"], p["rm"], p["rv"], EPS)
    # rows 2 / 3 are today's eval-path scale / shift bit for bit; rows 0 / 1 the running mean and 1/sqrt(var + eps)
    scale, shift = torch.empty(C, device=dev), torch.empty(C, device=dev)
    lib.call("mvs_bn_eval_affine", ops._p(p["gamma"]), ops._p(p["beta"]), ops._p(p["rm"]), ops._p(p["rv"]), EPS, C, ops._p(scale),
             ops._p(shift), ops._stream(raw_d))
    assert torch.equal(stats[2], scale) and torch.equal(stats[3], shift) and torch.equal(stats[0], p["rm"])
    assert torch.allclose(stats[1].cpu().double(), 1.0 / torch.sqrt(inp["rv"].double() + EPS), rtol=3e-7, atol=0)
    sc_ref = inp["gamma"].double() / torch.sqrt(inp["rv"].double() + EPS)
    assert torch.allclose(stats[2].cpu().double(), sc_ref, rtol=3e-7, atol=0)
    assert torch.allclose(stats[3].cpu().double(), inp["beta"].double() - inp["rm"].double() * sc_ref, rtol=0, atol=2e-6)
    if form == "prefilled":
        dy_d, slots = _prefilled(inp, C, rows, relu, dev, stats, raw_d)
    else:
        dy_d, slots = inp["dy"].to(dev).contiguous(memory_format=CL3), None
    dy = dy_d.cpu()
    y64, draw64, dgamma64, dbeta64, gskip64 = _truth64(inp, dy, relu, with_skip)
    # forward: the apply pass with rows 2 / 3 (+ skip after the ReLU)
    y = ops.bn_relu_fwd_frozen(raw_d, stats, inp["skip"].to(dev) if with_skip else None, relu=bool(relu)).cpu()
    assert float((y.double() - y64).abs().max()) <= 4 * 2.0 ** -23 * float(y64.abs().max() + 50.0)
    if with_skip:
        assert torch.equal(gskip64, dy.double())        # the skip source receives dy unchanged (the caller passes it on)
    if form == "none":
        draw, dgamma, dbeta = ops.bn_relu_bwd_frozen(dy_d, raw_d, stats, relu=bool(relu), want_affine=False)
        assert dgamma is None and dbeta is None
    else:
        draw, dgamma, dbeta = ops.bn_relu_bwd_frozen(dy_d, raw_d, stats, slots, form == "prefilled", relu=bool(relu))
    # draw: bit-identical to scale * dyh in fp32, same order (mask first, one multiplication)
    st = stats.cpu()
    v = lambda t: t.view(1, C, 1, 1, 1)
    mask = (inp["raw"].double() * v(st[2]).double() + v(st[3]).double() > 0) if relu else torch.ones_like(dy, dtype=torch.bool)
    expect = v(st[2]) * torch.where(mask, dy, torch.zeros_like(dy))
    assert torch.equal(draw.cpu(), expect)
    assert bool((draw.cpu()[0, 3][inp["raw"][0, 3] == 0] == 0).all()) or not relu
    assert torch.allclose(draw.cpu().double(), draw64, rtol=1e-6, atol=1e-6)
    if form != "none":
        print("frozen bn C=%d rows=%d relu=%d %s: dgamma err %.3e dbeta err %.3e" % (
            C, rows, relu, form, float((dgamma.cpu().double() - dgamma64).abs().max()), float((dbeta.cpu().double() - dbeta64).abs().max())))
        assert torch.allclose(dgamma.cpu().double(), dgamma64, rtol=2e-4, atol=2e-2)
        assert torch.allclose(dbeta.cpu().double(), dbeta64, rtol=2e-4, atol=2e-2)
        if relu:
            assert float(dbeta.cpu()[2]) == 0.0 and float(dgamma.cpu()[2]) == 0.0      # the channel that is negative everywhere


# ------------------------------------------------------------------------------------------------------------------------
# blocks, 3-D and 2-D, against the stock modules
# ------------------------------------------------------------------------------------------------------------------------
def _set_mode(block, bn, mode):
    if mode == "idiom":
        block.train()
        bn.eval()
    else:
        block.eval()


def _randomise_bn(bn, g):
    with torch.no_grad():
        bn.weight.copy_(0.5 + torch.rand(bn.num_features, generator=g))
        bn.bias.copy_(torch.randn(bn.num_features, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(bn.num_features, generator=g) * 0.2)
        bn.running_var.copy_(0.5 + torch.rand(bn.num_features, generator=g))
        bn.num_batches_tracked.fill_(7)


def _stock(conv, bn, dtype):
    conv, bn = copy.deepcopy(conv).cpu().to(dtype), copy.deepcopy(bn).cpu().to(dtype)
    bn.eval()
    return conv, bn


def _stock_run(conv, bn, x, skip, gy):
    x = x.detach().clone().to(conv.weight.dtype).requires_grad_(True)
    y = F.relu(bn(conv(x)))
    leaves = {"x": x}
    if skip is not None:
        leaves["skip"] = skip.detach().clone().to(conv.weight.dtype).requires_grad_(True)
        y = y + leaves["skip"]
    y.backward(gy.to(y.dtype))
    out = {k: t.grad for k, t in leaves.items()}
    out.update({"conv.weight": conv.weight.grad, "bn.weight": bn.weight.grad, "bn.bias": bn.bias.grad, "y": y.detach()})
    return out


BLOCKS_3D = {"conv_s2": (False, 8, 16, 2, (1, 8, 4, 8, 16)), "conv_s1": (False, 16, 16, 1, (1, 16, 3, 5, 18)),
             "deconv_s2_skip": (True, 16, 8, 2, (1, 16, 2, 4, 8))}


def block3d_case(dev, which, mode):
    """a 3-D block under the freeze idiom (mode "idiom") or in .eval() with autograd on (mode "eval"): output and every gradient
    vs the stock modules in fp64 with the stock fp32 modules as the yardstick; statistics and the batch counter untouched"""
    from mvs_amd.nn3d import ConvBnReLU3D, DeconvBnReLU3D
    transposed, cin, cout, stride, xs = BLOCKS_3D[which]
    g = torch.Generator().manual_seed(31 + cin + cout)
    block = DeconvBnReLU3D(cin, cout, stride=stride) if transposed else ConvBnReLU3D(cin, cout, stride=stride)
    conv, bn = (block[0], block[1]) if transposed else (block.conv, block.bn)
    _randomise_bn(bn, g)
    ref32, ref64 = _stock(conv, bn, torch.float32), _stock(conv, bn, torch.float64)
    block = block.to(dev)
    _set_mode(block, bn, mode)
    before = buffers_of(block)
    x = torch.randn(xs, generator=g)
    with torch.no_grad():
        yshape = ref32[0](x).shape
    skip = torch.randn(yshape, generator=g) if transposed else None
    gy = torch.randn(yshape, generator=g)
    xd = leaf(x, dev)
    sd = leaf(skip, dev) if skip is not None else None
    y = block(xd, skip=sd)
    y.backward(gy.to(dev))                                   # (.eval() + backward() raised before this path existed)
    assert_buffers_untouched(before, block, which + " " + mode)
    ours = {"x": xd.grad.cpu(), "conv.weight": conv.weight.grad.cpu(), "bn.weight": bn.weight.grad.cpu(), "bn.bias": bn.bias.grad.cpu(),
            "y": y.detach().cpu()}
    if sd is not None:
        ours["skip"] = sd.grad.cpu()
    assert_grads_as_accurate_as_fp32_reference(ours, _stock_run(*ref32, x, skip, gy), _stock_run(*ref64, x, skip, gy),
                                               what="frozen 3-D block %s (%s)" % (which, mode))
    # gamma / beta that want no gradient: the no-reduction pass; the other gradients are the same numbers
    for t in (bn.weight, bn.bias, conv.weight):
        t.grad = None
    bn.weight.requires_grad_(False)
    bn.bias.requires_grad_(False)
    xd2 = leaf(x, dev)
    block(xd2, skip=None if skip is None else skip.to(dev)).backward(gy.to(dev))
    assert bn.weight.grad is None and bn.bias.grad is None
    assert torch.equal(xd2.grad.cpu(), ours["x"]) and rel_l1(conv.weight.grad.cpu(), ours["conv.weight"]) < 1e-5
    assert_buffers_untouched(before, block, which + " " + mode)


def block3d_no_grad_case(dev, which):
    """Under no_grad (and whenever nothing requires a gradient) the eval output is the folded-epilogue convolution, bit for bit what
    the folded path gave before the frozen path existed: compared with the folded conv3d_forward(scale=, shift=) call directly."""
    from mvs_amd import ops
    from mvs_amd.nn3d import ConvBnReLU3D, DeconvBnReLU3D
    transposed, cin, cout, stride, xs = BLOCKS_3D[which]
    g = torch.Generator().manual_seed(77 + cin)
    block = DeconvBnReLU3D(cin, cout, stride=stride) if transposed else ConvBnReLU3D(cin, cout, stride=stride)
    conv, bn = (block[0], block[1]) if transposed else (block.conv, block.bn)
    _randomise_bn(bn, g)
    block = block.to(dev).eval()
    x = torch.randn(xs, generator=g).to(dev)
    lib = ops._lib_for(x)
    scale, shift = torch.empty(cout, device=dev), torch.empty(cout, device=dev)
    lib.call("mvs_bn_eval_affine", ops._p(bn.weight), ops._p(bn.bias), ops._p(bn.running_mean), ops._p(bn.running_var), float(bn.eps),
             cout, ops._p(scale), ops._p(shift), ops._stream(x))
    with torch.no_grad():
        folded, _ = ops.conv3d_forward(x, conv.weight, stride, transposed, scale=scale, shift=shift, relu=True)
        skip = torch.randn(folded.shape, generator=g).to(dev) if transposed else None
        if skip is not None:
            folded, _ = ops.conv3d_forward(x, conv.weight, stride, transposed, scale=scale, shift=shift, skip=skip, relu=True)
        y_ng = block(x, skip=skip)
    assert torch.equal(y_ng, folded)
    for p_ in block.parameters():                               # autograd on, nothing requires a gradient: still the folded path
        p_.requires_grad_(False)
    assert torch.equal(block(x, skip=skip), folded)
    for p_ in block.parameters():
        p_.requires_grad_(True)
    y_g = block(leaf(x, dev), skip=skip)      # with a gradient: raw convolution + apply pass, the same arithmetic
    assert y_g.requires_grad
    tol = 4 * 2.0 ** -23 * float(folded.abs().max() + scale.abs().max() * 8 + shift.abs().max())
    assert float((y_g.detach() - folded).abs().max()) <= tol
    if dev.type == "cpu":
        assert torch.equal(y_g.detach(), folded)                # (no contraction in the emulation: the very same fp32 operations)


def bn_relu_2d_case(dev, c, mode_groups):
    """ops.BnReLUFn(training=False) on a channels-last [B,C,H,W] activation vs stock BatchNorm2d.eval() + ReLU"""
    from mvs_amd import ops
    g = torch.Generator().manual_seed(5 + c)
    bn = nn.BatchNorm2d(c)
    _randomise_bn(bn, g)
    x = torch.randn(mode_groups, c, 9, 13, generator=g)
    gy = torch.randn(x.shape, generator=g)
    res = {}
    for dtype in (torch.float32, torch.float64):
        b = copy.deepcopy(bn).to(dtype).eval()
        xx = x.detach().clone().to(dtype).requires_grad_(True)
        yy = F.relu(b(xx))
        yy.backward(gy.to(dtype))
        res[dtype] = {"x": xx.grad, "bn.weight": b.weight.grad, "bn.bias": b.bias.grad, "y": yy.detach()}
    bn = bn.to(dev)
    before = buffers_of(bn)
    xd = leaf(x, dev, torch.channels_last)
    y = ops.BnReLUFn.apply(xd, bn.weight, bn.bias, bn.running_mean, bn.running_var, False, bn.eps, bn.momentum, mode_groups)
    y.backward(gy.to(dev))
    assert_buffers_untouched(before, bn, "BnReLUFn frozen")
    ours = {"x": xd.grad.cpu(), "bn.weight": bn.weight.grad.cpu(), "bn.bias": bn.bias.grad.cpu(), "y": y.detach().cpu()}
    assert_grads_as_accurate_as_fp32_reference(ours, res[torch.float32], res[torch.float64], what="BnReLUFn frozen C=%d" % c)
    with torch.no_grad():                                        # no gradient wanted: today's eval kernels, the same numbers
        y_ng = ops.BnReLUFn.apply(xd.detach(), bn.weight, bn.bias, bn.running_mean, bn.running_var, False, bn.eps, bn.momentum, mode_groups)
    assert torch.equal(y_ng, y.detach())


def block2d_case(dev, mode, cin=8, cout=16, k=3, stride=1):
    """the 2-D ConvBnReLU under the idiom / in .eval() with autograd on vs the stock modules; groups = 2 (two views)"""
    from mvs_amd.jdacs.models.module import ConvBnReLU
    g = torch.Generator().manual_seed(91 + cout + k)
    block = ConvBnReLU(cin, cout, k, stride, k // 2)
    _randomise_bn(block.bn, g)
    ref32, ref64 = _stock(block.conv, block.bn, torch.float32), _stock(block.conv, block.bn, torch.float64)
    block = block.to(dev).to(memory_format=torch.channels_last)
    _set_mode(block, block.bn, mode)
    before = buffers_of(block)
    x = torch.randn(2, cin, 12, 20, generator=g)
    with torch.no_grad():
        gy = torch.randn(ref32[0](x).shape, generator=g)
    xd = leaf(x, dev, torch.channels_last)
    y = block(xd, groups=2)
    y.backward(gy.to(dev))
    assert_buffers_untouched(before, block, "2-D block " + mode)
    ours = {"x": xd.grad.cpu(), "conv.weight": block.conv.weight.grad.cpu(), "bn.weight": block.bn.weight.grad.cpu(),
            "bn.bias": block.bn.bias.grad.cpu(), "y": y.detach().cpu()}
    assert_grads_as_accurate_as_fp32_reference(ours, _stock_run(*ref32, x, None, gy), _stock_run(*ref64, x, None, gy),
                                               what="frozen 2-D block (%s)" % mode)


# ------------------------------------------------------------------------------------------------------------------------
# the regularisers: one-node frozen form vs per-layer frozen form
# ------------------------------------------------------------------------------------------------------------------------
class call_log:
    """names of the C-ABI entry points called through lib.call while the context is open"""

    def __init__(self, lib):
        self.lib, self.names = lib, []

    def __enter__(self):
        self.orig = self.lib.call

        def call(name, *a, **k):
            self.names.append(name)
            return self.orig(name, *a, **k)
        self.lib.call = call
        return self

    def __exit__(self, *exc):
        del self.lib.call
        return False


TRAIN_MODE_KERNELS = ("bn_relu_fwd_slots", "bn_relu_bwd_slots", "bn_bwd_reduce_slots", "bn_stats_slots", "bn_finalize_slots")


def _regnet(which):
    if which == "mvs":
        from mvs_amd.jdacs.models.mvsnet import CostRegNet
        return CostRegNet(), R.OracleCostRegNet(), (1, 32, 8, 16, 16), "prob"
    from mvs_amd.jdacs_ms.models.network import CostRegNet
    return CostRegNet(), R.OracleCostRegNetMS(), (1, 16, 8, 16, 16), "prob0"


def _calibrated_regnet(which, g):
    net, oracle, xs, prob = _regnet(which)
    for m in net.modules():
        if isinstance(m, _BN):
            _randomise_bn(m, g)
            with torch.no_grad():
                m.running_mean.mul_(0.5)
    return net, oracle, xs, prob


def costreg_case(dev, which):
    """one-node frozen form (ops.UNetRegulariserFrozenFn) vs the per-layer frozen graph vs the oracle's stock modules (fp32
    yardstick, fp64 truth); no train-mode BatchNorm kernel and no C-entry pass in frozen mode; statistics untouched"""
    from mvs_amd import ops
    g = torch.Generator().manual_seed(17)
    net, oracle, xs, prob = _calibrated_regnet(which, g)
    x = torch.randn(xs, generator=g).abs() * 0.3
    with torch.no_grad():
        oracle.load_state_dict(net.state_dict())
        gy = torch.randn(oracle.eval()(x).shape, generator=g)
    refs = {}
    for dtype in (torch.float32, torch.float64):
        o = freeze_batchnorm(copy.deepcopy(oracle).to(dtype))
        xx = x.detach().clone().to(dtype).requires_grad_(True)
        yy = o(xx)
        yy.backward(gy.to(dtype))
        refs[dtype] = {k: p.grad for k, p in o.named_parameters()}
        refs[dtype].update(x=xx.grad, y=yy.detach())
    net = freeze_batchnorm(net.to(dev))
    lib = ops._lib_for(x.to(dev))
    before = buffers_of(net)
    res = {}
    for fused in (True, False):
        net.zero_grad(set_to_none=True)
        xd = leaf(x, dev)
        old = ops.FUSED_REGULARISER
        ops.FUSED_REGULARISER = fused
        try:
            lib.launch_trace()
            with call_log(lib) as log:
                y = net(xd)
                fwd_trace = lib.launch_trace()
                y.backward(gy.to(dev).view_as(y))
                bwd_trace = lib.launch_trace()
        finally:
            ops.FUSED_REGULARISER = old
        if dev.type == "cuda":
            torch.cuda.synchronize()
        for name in log.names:
            assert name not in ("mvs_unet_fwd", "mvs_unet_bwd") and not name.endswith("_slots"), name
        for label in fwd_trace + bwd_trace:
            assert label not in TRAIN_MODE_KERNELS, label
        # (the launch trace is per thread and the autograd engine runs a device's backward on a thread of its own: the C-ABI call
        #  log covers the backward pass everywhere, the trace where the backward ran on this thread)
        assert "bn_frozen_stats" in fwd_trace and "bn_relu_fwd" in fwd_trace and "mvs_bn_relu_bwd_frozen" in log.names
        assert "bn_relu_bwd_frozen" in bwd_trace or dev.type != "cpu"
        assert_buffers_untouched(before, net, "%s regulariser fused=%s" % (which, fused))
        res[fused] = {k: p.grad.cpu() for k, p in net.named_parameters()}
        res[fused].update(x=xd.grad.cpu(), y=y.detach().cpu().view_as(refs[torch.float32]["y"]))
        assert_grads_as_accurate_as_fp32_reference(res[fused], refs[torch.float32], refs[torch.float64],
                                                   what="frozen %s regulariser, %s" % (which, "one node" if fused else "per layer"))
    assert torch.equal(res[True]["y"], res[False]["y"])           # the same forward kernels in the same order
    return res


def costreg_mixed_case(dev, which):
    """one BatchNorm left in train mode: the per-layer graph runs, and only that module's statistics and counter move"""
    from mvs_amd import ops
    g = torch.Generator().manual_seed(23)
    net, _, xs, _ = _calibrated_regnet(which, g)
    net = freeze_batchnorm(net.to(dev))
    live = "conv1.bn"
    net.conv1.bn.train()
    lib = ops._lib_for(torch.zeros(1, device=dev))
    before = buffers_of(net)
    x = leaf(torch.randn(xs, generator=g).abs() * 0.3, dev)
    with call_log(lib) as log:
        y = net(x)
        y.sum().backward()
    assert not net._one_node()
    assert "mvs_unet_fwd" not in log.names and log.names.count("mvs_bn_relu_fwd_slots") == 1 and log.names.count("mvs_bn_relu_bwd_slots") == 1
    after = buffers_of(net)
    for k, v in before.items():
        if k.startswith(live):
            assert not torch.equal(v, after[k]), k
        else:
            assert torch.equal(v, after[k]), k
    assert int(after[live + ".num_batches_tracked"]) == int(before[live + ".num_batches_tracked"]) + 1
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())


# ------------------------------------------------------------------------------------------------------------------------
# whole models vs the fixtures written from the live reference (tests/golden/make_golden_frozen_bn.py)
# ------------------------------------------------------------------------------------------------------------------------
def _weights(depth):
    return torch.linspace(0.5, 1.5, depth.numel(), dtype=depth.dtype, device=depth.device).view_as(depth)


def _mvs_state(g6):
    sd = state_dict_from(g6)
    sd.update({k[4:]: v for k, v in g6.items() if k.startswith("cal.")})
    return sd


_MVS_TRUTH = {}


def mvsnet_truth():
    """fp64 oracle under the same idiom on g6's inputs, weights and calibrated statistics (computed once)"""
    if not _MVS_TRUTH:
        g6 = load_golden("g6_mvsnet_e2e")
        o = R.OracleMVSNet(refine=False)
        o.load_state_dict(_mvs_state(g6))
        o = freeze_batchnorm(o.double())
        imgs = g6["imgs"].double().requires_grad_(True)
        out = o(imgs, g6["proj"].double(), g6["depth_values"].double())
        (out["depth"] * _weights(out["depth"])).mean().backward()
        _MVS_TRUTH.update({k: p.grad for k, p in o.named_parameters()})
        _MVS_TRUTH["imgs"] = imgs.grad
    return _MVS_TRUTH


def mvsnet_case(dev, mode="idiom", affine_grads=True):
    from mvs_amd.jdacs.models.mvsnet import MVSNet
    g6, g18 = load_golden("g6_mvsnet_e2e"), load_parts("g18_frozen_bn_mvs")
    net = MVSNet(refine=False)
    net.load_state_dict(_mvs_state(g6))
    net = net.to(dev)
    if mode == "idiom":
        freeze_batchnorm(net)
    else:
        net.eval()
    if not affine_grads:
        for m in net.modules():
            if isinstance(m, _BN):
                m.weight.requires_grad_(False)
                m.bias.requires_grad_(False)
    imgs = leaf(g6["imgs"], dev)
    out = net(imgs, g6["proj"].to(dev), g6["depth_values"].to(dev))
    (out["depth"] * _weights(out["depth"])).mean().backward()
    depth = out["depth"].detach().cpu()
    print("frozen MVSNet (%s): depth rel_l1 vs fixture %.3e, vs g6.eval_depth %.3e" % (mode, rel_l1(depth, g18["depth"]), rel_l1(depth, g6["eval_depth"])))
    assert rel_l1(depth, g18["depth"]) < 1e-3
    for k, v in g18.items():                                   # the running statistics: the fixture's copy, bit for bit
        if k.startswith("after."):
            assert torch.equal(net.state_dict()[k[6:]].cpu(), v), k
    truth = mvsnet_truth()
    names = [k for k, p in net.named_parameters() if not k.endswith("prob.bias") and p.requires_grad]
    ours = {k: p.grad.cpu() for k, p in net.named_parameters() if k in names}
    ours["imgs"] = imgs.grad.cpu()
    ref32 = {k: g18["grad." + k] for k in names}
    ref32["imgs"] = g18["grad_imgs"]
    assert_grads_as_accurate_as_fp32_reference(ours, ref32, {k: truth[k] for k in ours}, what="frozen MVSNet (%s) vs g18" % mode)
    if not affine_grads:
        for m in net.modules():
            if isinstance(m, _BN):
                assert m.weight.grad is None and m.bias.grad is None
    return ours


def cvp_case(dev):
    from mvs_amd.jdacs_ms.models.network import CVPMVSNet
    g7, g18 = load_golden("g7_cvpmvsnet_e2e"), load_parts("g18_frozen_bn_cvp")
    sd = state_dict_from(g7)
    sd.update({k[4:]: v for k, v in g18.items() if k.startswith("cal.")})
    keys = ("ref_img", "src_imgs", "ref_in", "src_in", "ref_ex", "src_ex", "depth_min", "depth_max")
    args = R.cvp_args(nsrc=2, nscale=2, mode="train")
    loss = lambda o: sum((d * _weights(d)).mean() for d in o["depth_est_list"])
    o64 = R.OracleCVPMVSNet(args)
    o64.load_state_dict(sd, strict=False)
    o64 = freeze_batchnorm(o64.double())
    ins64 = [g7[k].double() for k in keys]
    ins64[0].requires_grad_(True)
    ins64[1].requires_grad_(True)
    loss(o64(*ins64)).backward()
    truth = {k: p.grad for k, p in o64.named_parameters()}
    truth.update(ref_img=ins64[0].grad, src_imgs=ins64[1].grad)
    net = CVPMVSNet(args)
    net.load_state_dict(sd, strict=False)
    net = freeze_batchnorm(net.to(dev))
    ins = [g7[k].to(dev) for k in keys]
    ins[0], ins[1] = leaf(ins[0], dev), leaf(ins[1], dev)
    out = net(*ins)
    loss(out).backward()
    for i in (0, 1):
        assert rel_l1(out["depth_est_list"][i].detach().cpu(), g18["depth%d" % i]) < 1e-3
    for k, v in g18.items():
        if k.startswith("after."):
            assert torch.equal(net.state_dict()[k[6:]].cpu(), v), k
    names = [k for k, _ in net.named_parameters() if not k.endswith("prob0.bias")]
    ours = {k: p.grad.cpu() for k, p in net.named_parameters() if k in names}
    ours.update(ref_img=ins[0].grad.cpu(), src_imgs=ins[1].grad.cpu())
    ref32 = {k: g18["grad." + k] for k in names}
    ref32.update(ref_img=g18["grad_ref_img"], src_imgs=g18["grad_src_imgs"])
    assert_grads_as_accurate_as_fp32_reference(ours, ref32, {k: truth[k] for k in ours}, what="frozen CVP-MVSNet vs g18")
