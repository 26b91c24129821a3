"""Train-mode BatchNorm (+ReLU, + skip after the ReLU) of csrc/bn.hip, kernel by kernel: the cases shared by tests/test_bn_train.py
(CPU emulation of the kernel sources) and tests/test_gpu_bn_train.py (the same cases on the device).

Pipeline under test, on a channels-last activation of G groups x Vg rows x C channels:
    mvs_bn_stats_slots      (sum x, sum x^2) per channel into fp64 slot rows [G, nslots, 2, C]
    mvs_bn_relu_fwd_slots   prologue: slot totals -> mean / invstd / scale / shift (stats [G, 4, C]) + running statistics;  y
    mvs_bn_finalize_slots   that prologue alone
    mvs_bn_bwd_reduce_slots (sum dyh, sum dyh*xhat), dyh = dy * [x*scale + shift > 0]
    mvs_bn_relu_bwd_slots   prologue: dgamma / dbeta (summed over the groups);  dx = scale*(dyh - mean dyh - xhat * mean dyh*xhat)
and beside them mvs_bn_eval_affine and mvs_bn_relu_fwd.

Three evaluations on the CPU, none of them produced by the code under test:
    truth  fp64 autograd of relu?(F.batch_norm(x, rm, rv, gamma, beta, training=True, momentum, eps)) (+ skip), called once per group
           in group order on the shared running buffers ("G successive BatchNorm calls", ops.BnReLUFn).  One row per group
           (Vg == 1): torch refuses ("Expected more than 1 value per channel"), so the truth is written by hand: mean = x, biased
           variance = 0 and the running_var update uses 0, which is what bn_fwd_slots_kernel documents (count > 1 ? unbiased : var).
    A      the same expression in fp32 with stock ops.
    B      the project's own formula in plain torch: per-channel fp32 x.sum / (x*x).sum (backward: fp32 sums of dyh and dyh*xhat),
           finished in fp64 as the kernel comments describe (E[x^2] - mean^2, clamped at 0), applied in fp32.  What the scheme can
           deliver.

Criteria:
    y, dx, skip gradient   conftest.assert_as_accurate_as_fp32_reference(ours, A, truth), default slack 4 and floor.
    everything else        err_ours <= 4 * max(err_A, err_B) + one fp32 ulp of the tensor's largest magnitude (max abs errors against
                           the truth; 4 = the "same order" factor of conftest.py; slot totals have no A).  Each row of stats
                           (mean, invstd, scale, shift) is a tensor of its own: their magnitudes differ by orders.
    conditioning sweep     the second inequality for every tensor, y and dx included: the kernel must be as good as its formula allows
                           at every mean/std ratio; against A alone the sum-of-squares scheme cannot hold at ratios 4 and 32.

On the ReLU mask.  Where the mask is closed the FROZEN backward gives dx == 0; the train-mode one does not: dx there is
-scale*(mean dyh + xhat * mean dyh*xhat), in the fp64 truth as in the kernel.  What is exact in train mode and asserted here: y == 0 (before
the skip add) exactly where the fp64 mask is closed and > 0 where it is open, dx == 0 on the channel that is closed everywhere (both
sums are 0) and its dgamma == dbeta == 0.  A single element whose mask the kernel got wrong puts an error of |scale*dy| ~ 1 on dx, which
the accuracy criterion (errors ~ 1e-6) cannot miss.  So that the kernel and not the rounding decides the mask, no pre-activation of
the inputs lies within 1e-3 of zero (asserted on the CPU for every case; nothing is excluded from any comparison)."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_as_accurate_as_fp32_reference

EPS = float(np.float32(1e-5))      # the kernels take eps as a float: truth, A and B use that very number
MOM = 0.1
SLACK = 4.0
CHANNELS = (4, 8, 16, 32, 64)
DIMS = {105: (3, 5, 7), 4096: (16, 16, 16)}     # 105 rows: n4 below one workgroup at C = 4 and no multiple of 256
GAMMA0_CH, CLOSED_CH, CONST_CH = 1, 2, 3        # gamma = 0 / beta = -50 (ReLU closed everywhere) / constant over all rows (var == 0)
# The constant channel: n * 2^-8 and n * 2^-16 are exact in fp32 for every n used here, so var is exactly 0 and invstd = 1/sqrt(eps) = 316.
# The value and the channel's dy are scaled by 2^-8 ~ sqrt(eps) so that x*scale and dx stay O(1) like every other channel: the floor of
# conftest's criterion is an absolute 2e-6, less than one fp32 ulp of a value of 316, and all rows of this channel are the same number,
# so whether the stock fp32 ops happen to round that one number exactly would decide the case.
CONST_VALUE = 2.0 ** -8
CAP_STATS, CAP_REDUCE, CAP_APPLY = 512, 1024, 2048   # workgroup caps of bn_stats_slots / bn_bwd_reduce_slots / the apply passes
ROWS_ALL_CAPS = 262181      # C = 8: n4 = 524362 = 2048*256 + 74: every kernel takes a ragged second (third, fifth) grid-stride pass
ROWS_STATS_CAP = 65573      # C = 8: n4 = 131146 = 512*256 + 74: only bn_stats_slots does


def ulp32(t):
    """one fp32 ulp of the tensor's largest magnitude"""
    m = float(t.abs().max()) if t.numel() else 0.0
    return float(np.spacing(np.float32(m))) if m > 0 else float(np.spacing(np.float32(0)))


# ------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------
class Inputs:
    pass


_INPUTS = {}


def _z64(x, gamma, beta, G):
    """fp64 pre-activation z [V, C] and the per-row scale of the train-mode normalisation, group by group"""
    V, C = x.shape
    xg = x.double().view(G, V // G, C)
    mean = xg.mean(1, keepdim=True)
    var = ((xg - mean) ** 2).mean(1, keepdim=True)
    sc = gamma.double().view(1, 1, C) / torch.sqrt(var + EPS)
    z = (xg - mean) * sc + beta.double().view(1, 1, C)
    return z.reshape(V, C), sc.expand(G, V // G, C).reshape(V, C), var.view(G, C)


def inputs(C, rows, G=1, ratio=None):
    """Seeded per (C, rows) like frozen_bn_cases.kernel_inputs; rows [V = G*Vg, C] row-major (the channels-last memory image).
    Channel means within +-1 std (ratio=None) or exactly ratio * std with alternating sign (the conditioning sweep).  Channel 1 has
    gamma = 0, channel 2 a beta so negative that the ReLU is closed everywhere, channel 3 is constant over all rows.  Elements whose
    fp64 pre-activation is within 1e-3 of zero (and whose scale is not 0) are moved away from zero, z recomputed (the statistics move
    with x), at most three times; then the construction is asserted."""
    key = (C, rows, G, ratio)
    if key in _INPUTS:
        return _INPUTS[key]
    assert rows % G == 0 and C > CONST_CH
    g = torch.Generator().manual_seed(1000 * C + rows)
    inp = Inputs()
    inp.C, inp.V, inp.G, inp.Vg = C, rows, G, rows // G
    std = 0.5 + torch.rand(C, generator=g)
    if ratio is None:
        mean = (2 * torch.rand(C, generator=g) - 1) * std
    else:
        mean = float(ratio) * std * torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
    x = torch.randn(rows, C, generator=g)
    if rows // G > 1:         # every group's SAMPLE has this mean and std, not just the distribution (two rows: |mean|/std is unbounded)
        xd = x.double().view(G, rows // G, C)
        x = ((xd - xd.mean(1, keepdim=True)) / xd.std(1, unbiased=False, keepdim=True)).float().view(rows, C)
    x = x * std + mean
    x[:, CONST_CH] = CONST_VALUE
    gamma = 0.5 + torch.rand(C, generator=g)
    beta = torch.randn(C, generator=g) * 0.3
    beta = torch.where(beta.abs() < 0.05, torch.where(beta < 0, -0.05, 0.05), beta)    # (Vg == 1: z == beta)
    gamma[GAMMA0_CH] = 0.0
    beta[CLOSED_CH] = -50.0
    inp.rm, inp.rv = torch.randn(C, generator=g) * 0.5, 0.5 + torch.rand(C, generator=g)
    for _ in range(3):
        z, sc, _ = _z64(x, gamma, beta, G)
        near = (z.abs() < 1e-3) & (sc != 0)
        if not bool(near.any()):
            break
        step = torch.where(z >= 0, 1.0, -1.0) * 2e-3 / sc.abs().clamp_min(1e-3)
        x = torch.where(near, x.double() + step, x.double()).float()
    z, sc, var = _z64(x, gamma, beta, G)
    assert not bool(((z.abs() < 1e-3) & (sc != 0)).any()), "a pre-activation within 1e-3 of zero is left"
    assert bool((z[:, CLOSED_CH] < 0).all()), "the closed channel is open somewhere"
    assert bool((var[:, CONST_CH] == 0).all()) and bool((x[:, CONST_CH] == CONST_VALUE).all()), "the constant channel is not constant"
    inp.x, inp.gamma, inp.beta = x, gamma, beta
    inp.open64 = z > 0
    inp.dy = torch.randn(rows, C, generator=g)
    inp.dy[:, CONST_CH] *= CONST_VALUE
    inp.skip = torch.randn(rows, C, generator=g)
    _INPUTS[key] = inp
    return inp


# ------------------------------------------------------------------------------------------------------------------------
# truth, yardstick A, yardstick B
# ------------------------------------------------------------------------------------------------------------------------
_REFS = {}


def stock(inp, dtype, relu, with_skip):
    """truth (float64) / yardstick A (float32): stock ops, one batch_norm call per group on the shared running buffers"""
    key = (id(inp), dtype, relu, with_skip)
    if key in _REFS:
        return _REFS[key]
    G, Vg, C = inp.G, inp.Vg, inp.C
    x, gamma, beta, skip = (t.detach().clone().to(dtype).requires_grad_(True) for t in (inp.x, inp.gamma, inp.beta, inp.skip))
    rm, rv = inp.rm.clone().to(dtype), inp.rv.clone().to(dtype)
    ys, stats = [], []
    for g in range(G):
        xg = x[g * Vg:(g + 1) * Vg]
        if Vg == 1:
            # by hand (see the module docstring): mean = x, biased variance 0, running_var takes 0.  Written as x*w + (beta - mean*w),
            # w = gamma * invstd: the form ATen's CPU kernel applies at every count > 1, so that A is the same yardstick at count 1
            mean = xg.mean(0, keepdim=True)
            var = ((xg - mean) ** 2).mean(0, keepdim=True)
            w = gamma / torch.sqrt(var + EPS)
            ys.append(xg * w + (beta - mean * w))
            with torch.no_grad():
                rm.mul_(1 - MOM).add_(MOM * mean[0])
                rv.mul_(1 - MOM).add_(MOM * var[0])
        else:
            ys.append(F.batch_norm(xg, rm, rv, gamma, beta, True, MOM, EPS))
        with torch.no_grad():
            mean = xg.mean(0)
            invstd = 1.0 / torch.sqrt(((xg - mean) ** 2).mean(0) + EPS)
            sc = gamma * invstd
            stats.append(torch.stack([mean, invstd, sc, beta - mean * sc]))
    z = torch.cat(ys, 0)
    y = F.relu(z) if relu else z
    if with_skip:
        y = y + skip
    y.backward(inp.dy.to(dtype))
    out = dict(y=y.detach(), stats=torch.stack(stats).detach(), rm=rm, rv=rv, dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad,
               gskip=skip.grad if with_skip else None)
    if dtype == torch.float64:
        with torch.no_grad():
            xd = inp.x.double().view(G, Vg, C)
            out["tot_f"] = torch.stack([xd.sum(1), (xd * xd).sum(1)], 1)                    # [G, 2, C]
            st = out["stats"]
            dyh = inp.dy.double().view(G, Vg, C) * ((z.detach().view(G, Vg, C) > 0) if relu else 1.0)
            xhat = (xd - st[:, 0:1]) * st[:, 1:2]
            out["tot_b"] = torch.stack([dyh.sum(1), (dyh * xhat).sum(1)], 1)
    _REFS[key] = out
    return out


def formula(inp, relu, with_skip):
    """yardstick B: the statistic-slot scheme in plain torch (fp32 sums, fp64 finish, fp32 apply), kernel comments of csrc/bn.hip"""
    key = (id(inp), "B", relu, with_skip)
    if key in _REFS:
        return _REFS[key]
    G, Vg, C = inp.G, inp.Vg, inp.C
    f32 = torch.float32
    x = inp.x.view(G, Vg, C)
    dy = inp.dy.view(G, Vg, C)
    s1, s2 = x.sum(1), (x * x).sum(1)                                 # fp32 sums [G, C]
    count = float(Vg)
    rm, rv = inp.rm.clone(), inp.rv.clone()
    mom = torch.tensor(MOM, dtype=f32)
    stats, ys, dxs, tb = [], [], [], []
    for g in range(G):
        mean = s1[g].double() / count
        var = (s2[g].double() / count - mean * mean).clamp_min(0.0)
        unbiased = var * count / (count - 1.0) if count > 1.0 else var
        rm = (1.0 - mom) * rm + mom * mean.to(f32)
        rv = (1.0 - mom) * rv + mom * unbiased.to(f32)
        eps = float(np.float32(EPS))
        invstd = (1.0 / torch.sqrt(var + eps)).to(f32)
        sc = inp.gamma * invstd
        sh = inp.beta - mean.to(f32) * sc
        mu = mean.to(f32)
        stats.append(torch.stack([mu, invstd, sc, sh]))
        z = x[g] * sc + sh
        y = F.relu(z) if relu else z
        ys.append(y + inp.skip.view(G, Vg, C)[g] if with_skip else y)
        dyh = torch.where(z > 0, dy[g], torch.zeros_like(dy[g])) if relu else dy[g]
        xhat = (x[g] - mu) * invstd
        t1, t2 = dyh.sum(0), (dyh * xhat).sum(0)                       # fp32 sums
        tb.append(torch.stack([t1, t2]))
        inv = torch.tensor(1.0, dtype=f32) / torch.tensor(count, dtype=f32)
        dxs.append(sc * (dyh - t1 * inv - xhat * (t2 * inv)))
    tb = torch.stack(tb)
    out = dict(y=torch.cat(ys, 0), stats=torch.stack(stats), rm=rm, rv=rv, dx=torch.cat(dxs, 0),
               dbeta=tb[:, 0].double().sum(0).to(f32), dgamma=tb[:, 1].double().sum(0).to(f32),
               tot_f=torch.stack([s1, s2], 1).double(), tot_b=tb.double())
    _REFS[key] = out
    return out


# ------------------------------------------------------------------------------------------------------------------------
# the record
# ------------------------------------------------------------------------------------------------------------------------
def _report_path():
    folder = os.environ.get("MVS_BN_REPORT", "")
    if not folder and os.environ.get("MVS_GRAD_REPORT"):
        folder = os.path.dirname(os.path.abspath(os.environ["MVS_GRAD_REPORT"]))
    return os.path.join(folder, "bn_parity_ratios.jsonl") if folder else ""


class Record:
    """per-tensor (ours, A, B, ratio) of one case; ratio = (err_ours - additive term) / yardstick, <= 4 iff the criterion holds.
    One JSON line per case into bn_parity_ratios.jsonl in the folder MVS_BN_REPORT names (or next to MVS_GRAD_REPORT's file); the
    device run's copy kept with the project is profiles/bn_parity_ratios.jsonl."""

    def __init__(self, case, dev):
        self.case, self.suite, self.tensors, self.bad = case, ("device" if dev.type == "cuda" else "emulation"), {}, []

    def add(self, name, e_o, e_a, e_b, yard, add, judge=True):
        over = max(0.0, e_o - add)
        ratio = over / yard if yard > 0 else (0.0 if over == 0 else float("inf"))
        self.tensors[name] = dict(ours=e_o, A=e_a, B=e_b, ratio=ratio)
        print("%s %s: ours %.3e  A %s  B %s  ratio %.3f" % (self.case, name, e_o, "-" if e_a is None else "%.3e" % e_a,
                                                           "-" if e_b is None else "%.3e" % e_b, ratio))
        if judge and not e_o <= SLACK * yard + add:
            self.bad.append("%s: err %.3e > %g * %.3e + %.3e" % (name, e_o, SLACK, yard, add))

    def finish(self):
        worst = max(self.tensors, key=lambda k: self.tensors[k]["ratio"])
        row = dict(case=self.case, suite=self.suite, slack_allowed=SLACK, worst_tensor=worst, **self.tensors[worst], tensors=self.tensors)
        out = _report_path()
        if out:
            try:
                with open(out, "a") as fh:
                    fh.write(json.dumps(row) + "\n")
            except OSError:
                pass
        assert not self.bad, "%s: %s" % (self.case, "; ".join(self.bad))


def _err(a, t):
    return float((a.double() - t.double()).abs().max()) if t.numel() else 0.0


def check_sums(rec, name, ours, a, b, truth):
    """err_ours <= 4 * max(err_A, err_B) + one fp32 ulp of the tensor's largest magnitude"""
    e_o, e_a, e_b = _err(ours, truth), (None if a is None else _err(a, truth)), _err(b, truth)
    assert bool(torch.isfinite(ours).all()), "%s %s: not finite" % (rec.case, name)
    rec.add(name, e_o, e_a, e_b, max(e_a or 0.0, e_b), ulp32(truth))


def check_elementwise(rec, name, ours, a, b, truth):
    """conftest.assert_as_accurate_as_fp32_reference with its defaults (max and mean error against A alone); B recorded only"""
    assert bool(torch.isfinite(ours).all()), "%s %s: not finite" % (rec.case, name)
    t = truth.float()
    rec.add(name, _err(ours, t), _err(a, t), None if b is None else _err(b, t), _err(a, t), 2e-6, judge=False)    # (judged below)
    assert_as_accurate_as_fp32_reference(ours.float(), a, truth, what="%s %s" % (rec.case, name))


# ------------------------------------------------------------------------------------------------------------------------
# the kernels
# ------------------------------------------------------------------------------------------------------------------------
def _view(t, dev, G, sp):
    """rows [G*Vg, C] -> a channels-last [G, C, *sp] tensor on the device (no copy of the layout: the rows ARE the memory image)"""
    n = len(sp)
    return t.to(dev).view(G, *sp, t.shape[1]).permute(0, n + 1, *range(1, n + 1))


def _rows(t):
    n = t.dim() - 2
    return t.permute(0, *range(2, n + 2), 1).reshape(-1, t.shape[1]).cpu()


def _spatial(inp, ndim, dims):
    if dims is not None:
        assert math.prod(dims) == inp.Vg and len(dims) == ndim - 2
        return tuple(dims)
    return (1,) * (ndim - 3) + (inp.Vg,)


def workgroups(n4, cap):
    return max(1, min((n4 + 255) // 256, cap))


def run_kernels(dev, inp, relu, with_skip, nslots=None, ndim=5, dims=None):
    """stats -> forward (+ finalize, twice) -> backward reduction -> backward apply; everything back on the CPU as rows [V, C].
    Exact properties are asserted here; the accuracy comparison is the caller's."""
    from mvs_amd import ops
    G, Vg, C = inp.G, inp.Vg, inp.C
    sp = _spatial(inp, ndim, dims)
    x_d, dy_d = _view(inp.x, dev, G, sp), _view(inp.dy, dev, G, sp)
    skip_d = _view(inp.skip, dev, G, sp) if with_skip else None
    gamma, beta = inp.gamma.to(dev), inp.beta.to(dev)
    lib = ops._lib_for(x_d)
    ns = ops.bn_nslots(lib, C) if nslots is None else nslots
    st = ops._stream(x_d)
    slots_f, slots_b = ops.stat_slots(x_d, G, ns, C, 2)
    assert tuple(slots_f.shape) == (G, ns, 2, C)
    lib.call("mvs_bn_stats_slots", ops._p(x_d), G, Vg, C, ops._p(slots_f), ns, st)
    rm, rv = inp.rm.clone().to(dev), inp.rv.clone().to(dev)
    y, stats = ops.bn_relu_fwd_slots(x_d, slots_f, gamma, beta, rm, rv, EPS, MOM, skip_d, relu=bool(relu), groups=G)
    # mvs_bn_finalize_slots on the same slots: stats and running statistics bit-identical to the forward prologue's ...
    rm2, rv2 = inp.rm.clone().to(dev), inp.rv.clone().to(dev)
    stats2 = ops.bn_finalize_slots(slots_f, gamma, beta, rm2, rv2, EPS, MOM, Vg)
    assert torch.equal(stats2, stats) and torch.equal(rm2, rm) and torch.equal(rv2, rv), "finalize differs from the forward prologue"
    # ... and without running buffers: stats all the same, no buffer written
    keep = [t.clone() for t in (rm, rv, rm2, rv2, gamma, beta)]
    stats3 = ops.bn_finalize_slots(slots_f, gamma, beta, None, None, EPS, MOM, Vg)
    assert torch.equal(stats3, stats)
    assert all(torch.equal(a, b) for a, b in zip(keep, (rm, rv, rm2, rv2, gamma, beta))), "finalize(None, None) wrote a buffer"
    lib.call("mvs_bn_bwd_reduce_slots", ops._p(dy_d), ops._p(x_d), ops._p(stats), int(relu), G, Vg, C, ops._p(slots_b), ns, st)
    slots_b_before = slots_b.clone()
    dx, dgamma, dbeta = ops.bn_relu_bwd_slots(dy_d, x_d, stats, slots_b, True, relu=bool(relu), groups=G)
    assert torch.equal(slots_b, slots_b_before)                          # the apply pass only reads them
    n4 = Vg * C // 4
    sf, sb = slots_f.cpu(), slots_b.cpu()
    for s, cap, what in ((sf, CAP_STATS, "bn_stats_slots"), (sb, CAP_REDUCE, "bn_bwd_reduce_slots")):
        used = min(ns, workgroups(n4, cap))                              # row = workgroup & (nslots - 1)
        assert bool((s[:, used:] == 0).all()), "%s: an unused slot row was written" % what
    assert bool((sf[:, :min(ns, workgroups(n4, CAP_STATS)), 1] > 0).all()), "bn_stats_slots: a slot row that a workgroup owns is empty"
    out = dict(y=_rows(y), stats=stats.cpu(), rm=rm.cpu(), rv=rv.cpu(), dx=_rows(dx), dgamma=dgamma.cpu(), dbeta=dbeta.cpu(),
               tot_f=sf.sum(1), tot_b=sb.sum(1), gskip=_rows(dy_d) if with_skip else None)
    # exact properties
    if relu:
        if not with_skip:
            assert bool((out["y"][~inp.open64] == 0).all()) and bool((out["y"][inp.open64] > 0).all()), "the ReLU mask differs from fp64's"
        assert bool((out["dx"][:, CLOSED_CH] == 0).all()), "dx on the channel that is closed everywhere"
        assert float(out["dgamma"][CLOSED_CH]) == 0.0 and float(out["dbeta"][CLOSED_CH]) == 0.0
        assert bool((out["tot_b"][:, :, CLOSED_CH] == 0).all())
    assert bool((out["stats"][:, 1, CONST_CH] == float(np.float32(1.0 / math.sqrt(float(np.float32(EPS)))))).all()), "var < 0 clamp / var == 0"
    assert bool((out["stats"][:, 0, CONST_CH] == CONST_VALUE).all())
    if with_skip:
        assert torch.equal(out["gskip"], inp.dy)                         # the skip source receives dy unchanged (the caller passes it on)
    return out


STAT_ROWS = ("mean", "invstd", "scale", "shift")


def compare(rec, inp, ours, relu, with_skip, sweep=False):
    t, a, b = stock(inp, torch.float64, relu, with_skip), stock(inp, torch.float32, relu, with_skip), formula(inp, relu, with_skip)
    check_sums(rec, "slot_totals_fwd", ours["tot_f"], None, b["tot_f"], t["tot_f"])
    for i, row in enumerate(STAT_ROWS):
        check_sums(rec, "stats." + row, ours["stats"][:, i], a["stats"][:, i], b["stats"][:, i], t["stats"][:, i])
    for k in ("rm", "rv"):
        check_sums(rec, k, ours[k], a[k], b[k], t[k])
    check_sums(rec, "slot_totals_bwd", ours["tot_b"], None, b["tot_b"], t["tot_b"])
    for k in ("dgamma", "dbeta"):
        check_sums(rec, k, ours[k], a[k], b[k], t[k])
    for k in ("y", "dx"):
        (check_sums if sweep else check_elementwise)(rec, k, ours[k], a[k], b[k], t[k])
    if with_skip:
        assert torch.equal(t["gskip"], inp.dy.double())
        check_elementwise(rec, "gskip", ours["gskip"], a["gskip"], None, t["gskip"])
    rec.finish()


def matrix_case(dev, C, rows, relu, with_skip):
    """case 1: slot rows as mvs_bn_slots recommends, one group, dims (3,5,7) / (16,16,16)"""
    inp = inputs(C, rows)
    ours = run_kernels(dev, inp, relu, with_skip, dims=DIMS[rows])
    compare(Record("matrix C=%d rows=%d relu=%d skip=%d" % (C, rows, relu, int(with_skip)), dev), inp, ours, relu, with_skip)


# C -> (a row count that launches fewer workgroups than any slot-row count > 1, one that launches 301: more than 256 rows -> they wrap)
SLOT_ROWS = {4: (105, 76801), 8: (105, 38405), 64: (105, 4803)}


def slot_rows_case(dev, C, which, many):
    """case 2: nslots 1 / recommended / 256.  256 rows of C = 4 are 2048 doubles, the boundary of bn_slot_totals' eight-load prologue;
    C = 8: 4096, C = 64: 32768 doubles, both in its tail loop."""
    from mvs_amd import ops
    rows = SLOT_ROWS[C][1 if many else 0]
    inp = inputs(C, rows)
    lib = ops._lib_for(torch.zeros(1, device=dev))
    ns = {"one": 1, "recommended": ops.bn_nslots(lib, C), "max": 256}[which]
    n4 = rows * C // 4
    if many:
        assert workgroups(n4, CAP_STATS) > 256
    else:
        assert workgroups(n4, CAP_APPLY) < ops.bn_nslots(lib, C)
    ours = run_kernels(dev, inp, 1, False, nslots=ns)
    compare(Record("slot rows C=%d nslots=%d rows=%d" % (C, ns, rows), dev), inp, ours, 1, False)


def grid_cap_case(dev, rows):
    """case 3: C = 8, n4 just over a workgroup cap * 256"""
    inp = inputs(8, rows)
    n4 = rows * 2
    assert n4 > CAP_STATS * 256 and n4 % 256 != 0 and (n4 > CAP_APPLY * 256) == (rows == ROWS_ALL_CAPS)
    ours = run_kernels(dev, inp, 1, True)
    compare(Record("grid caps C=8 rows=%d" % rows, dev), inp, ours, 1, True)


# (G, Vg, C, tensor rank): count == 1, count == 2, the owner's G == 1 shortcut and G == 2 on the same 6 rows, the largest G
GROUP_CASES = [(1, 6, 8, 5), (2, 3, 8, 5), (1, 6, 8, 4), (2, 3, 8, 4), (3, 2, 16, 4), (3, 35, 32, 5), (2, 1, 8, 5), (64, 1, 4, 4),
               (64, 2, 64, 5), (64, 5, 16, 4)]


def groups_case(dev, G, Vg, C, ndim):
    """case 4: running statistics == G successive updates, dgamma / dbeta == the sum over the groups (both in the truth)"""
    inp = inputs(C, G * Vg, G)
    for relu in (1, 0):
        ours = run_kernels(dev, inp, relu, False, ndim=ndim)
        if Vg == 1:          # mean = x: xhat == 0, y == beta, dx == 0 and dgamma == 0 exactly; running_var decays towards 0
            assert bool((ours["dx"] == 0).all()) and bool((ours["dgamma"] == 0).all())
            assert bool((ours["stats"][:, 0] == inp.x).all())
        compare(Record("groups G=%d Vg=%d C=%d %d-D relu=%d" % (G, Vg, C, ndim, relu), dev), inp, ours, relu, False)


def finalize_case(dev, C, rows, G):
    """case 5 (run_kernels asserts it in every other case as well): finalize == the forward prologue, bit for bit"""
    inp = inputs(C, rows, G)
    run_kernels(dev, inp, 1, False)


EVAL_CHANNELS = (1, 4, 63, 64, 65, 130)      # one thread, the edges of the 64-thread workgroup, a third workgroup


def eval_affine_case(dev, C):
    """case 6a: mvs_bn_eval_affine, scale = gamma / sqrt(rv + eps), shift = beta - rm * scale"""
    from mvs_amd import ops
    g = torch.Generator().manual_seed(40 + C)
    gamma, beta = 0.5 + torch.rand(C, generator=g), torch.randn(C, generator=g) * 0.3
    rm, rv = torch.randn(C, generator=g) * 0.5, 0.5 + torch.rand(C, generator=g)
    pad = 7                                                   # guard elements after the C-th: a thread past C must write nothing
    scale, shift = torch.full((C + pad,), -7.0, device=dev), torch.full((C + pad,), -7.0, device=dev)
    d = [t.to(dev) for t in (gamma, beta, rm, rv)]
    lib = ops._lib_for(d[0])
    lib.call("mvs_bn_eval_affine", *[ops._p(t) for t in d], EPS, C, ops._p(scale), ops._p(shift), ops._stream(d[0]))
    scale, shift = scale.cpu(), shift.cpu()
    assert bool((scale[C:] == -7.0).all()) and bool((shift[C:] == -7.0).all())
    rec = Record("eval affine C=%d" % C, dev)
    eps = float(np.float32(EPS))
    sc64 = gamma.double() / torch.sqrt(rv.double() + eps)
    sc32 = gamma / torch.sqrt(rv + torch.tensor(eps, dtype=torch.float32))
    check_sums(rec, "scale", scale[:C], sc32, sc32, sc64)
    check_sums(rec, "shift", shift[:C], beta - rm * sc32, beta - rm * sc32, beta.double() - rm.double() * sc64)
    rec.finish()


def eval_apply_case(dev, rows, relu, with_skip):
    """case 6b: mvs_bn_relu_fwd, y = relu?(x*scale + shift) (+ skip) with given fp32 scale / shift"""
    from mvs_amd import ops
    C = 8
    inp = inputs(C, rows)
    g = torch.Generator().manual_seed(rows)
    scale, shift = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.arange(C) % 3 == 0, -1.0, 1.0), torch.randn(C, generator=g) * 0.3
    sp = DIMS.get(rows) or (1, 1, rows)
    x_d = _view(inp.x, dev, 1, sp)
    skip_d = _view(inp.skip, dev, 1, sp) if with_skip else None
    y = torch.empty_like(x_d, memory_format=torch.channels_last_3d)
    lib = ops._lib_for(x_d)
    scale_d, shift_d = scale.to(dev), shift.to(dev)
    lib.call("mvs_bn_relu_fwd", ops._p(x_d), ops._p(scale_d), ops._p(shift_d), ops._p(skip_d), int(relu), rows, C, ops._p(y), ops._stream(x_d))

    def ref(dtype):
        z = inp.x.to(dtype) * scale.to(dtype) + shift.to(dtype)
        z = F.relu(z) if relu else z
        return z + inp.skip.to(dtype) if with_skip else z
    rec = Record("eval apply rows=%d relu=%d skip=%d" % (rows, relu, int(with_skip)), dev)
    check_elementwise(rec, "y", _rows(y), ref(torch.float32), None, ref(torch.float64))
    rec.finish()


def backward_twice_case(dev, ndim):
    """case 7: ops.BnReLUFn, backward twice through a retained graph: the wrapper re-zeroes the slot rows it used, so the second
    backward gives the first one's gradients and not the doubled sums"""
    from mvs_amd import ops
    G, Vg, C = 2, 240, 16
    inp = inputs(C, G * Vg, G)
    sp = (12, 20) if ndim == 4 else (2, 6, 20)
    x = _view(inp.x, dev, G, sp).detach().requires_grad_(True)
    gamma, beta = (t.detach().clone().to(dev).requires_grad_(True) for t in (inp.gamma, inp.beta))   # (.to() of a CPU tensor is the tensor)
    rm, rv = inp.rm.clone().to(dev), inp.rv.clone().to(dev)
    y = ops.BnReLUFn.apply(x, gamma, beta, rm, rv, True, EPS, MOM, G)
    gy = _view(inp.dy, dev, G, sp)
    first = torch.autograd.grad(y, (x, gamma, beta), gy, retain_graph=True)
    second = torch.autograd.grad(y, (x, gamma, beta), gy, retain_graph=True)
    t, a, b = stock(inp, torch.float64, 1, False), stock(inp, torch.float32, 1, False), formula(inp, 1, False)
    for n, (g1, g2) in enumerate(zip(first, second)):
        g1, g2 = g1.cpu(), g2.cpu()
        # (the fp64 atomics of two passes may land in another order: the last bit of a sum, not more)
        assert float((g2 - g1).abs().max()) <= 2 * ulp32(g1), "the second backward differs from the first"
        if n:
            assert float((g2 - 2 * g1).abs().max()) > 0.1 * float(g1.abs().max()), "the doubled sums"
    for tag, grads in (("first", first), ("second", second)):
        rec = Record("BnReLUFn %d-D backward %s" % (ndim, tag), dev)
        check_elementwise(rec, "y", _rows(y.detach()), a["y"], b["y"], t["y"])
        check_elementwise(rec, "dx", _rows(grads[0]), a["dx"], b["dx"], t["dx"])
        check_sums(rec, "dgamma", grads[1].cpu(), a["dgamma"], b["dgamma"], t["dgamma"])
        check_sums(rec, "dbeta", grads[2].cpu(), a["dbeta"], b["dbeta"], t["dbeta"])
        check_sums(rec, "rm", rm.cpu(), a["rm"], b["rm"], t["rm"])
        check_sums(rec, "rv", rv.cpu(), a["rv"], b["rv"], t["rv"])
        rec.finish()


def argument_checks_case(dev):
    """case 8: every bad argument returns non-zero and launches nothing (the all-NULL calls are tests/test_capi_symbols.py's)"""
    from mvs_amd import ops
    C, Vg, ns = 8, 64, 16
    x = torch.randn(1, C, 4, 4, 4).to(dev).contiguous(memory_format=torch.channels_last_3d)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    lib = ops._lib_for(x)
    (slots,) = ops.stat_slots(x, 1, 256, 64, 1)                      # room for every shape tried below
    v = torch.ones(64, device=dev)
    stats = torch.zeros(4 * 64, device=dev)
    p, s = ops._p, ops._stream(x)
    with pytest.raises(ValueError, match="4/8/16/32/64"):
        ops.bn_nslots(lib, 12)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    lib.launch_trace()

    def stats_slots(C=C, G=1, ns=ns, x_=x, slots_=slots):
        return lib.raw("mvs_bn_stats_slots", p(x_), G, Vg, C, p(slots_), ns, s)

    def fwd(C=C, G=1, ns=ns, rm=v, rv=v, **nul):
        a = dict(x=x, slots=slots, gamma=v, beta=v, stats=stats, y=y)
        a.update(nul)
        return lib.raw("mvs_bn_relu_fwd_slots", p(a["x"]), p(a["slots"]), ns, G, Vg, C, p(a["gamma"]), p(a["beta"]), EPS, MOM, p(rm), p(rv),
                       None, 1, p(a["stats"]), p(a["y"]), s)

    def fin(C=C, G=1, ns=ns, rm=v, rv=v, **nul):
        a = dict(slots=slots, gamma=v, beta=v, stats=stats)
        a.update(nul)
        return lib.raw("mvs_bn_finalize_slots", p(a["slots"]), ns, G, Vg, C, p(a["gamma"]), p(a["beta"]), EPS, MOM, p(rm), p(rv), p(a["stats"]), s)

    def red(C=C, G=1, ns=ns, **nul):
        a = dict(dy=x, x=x, stats=stats, slots=slots)
        a.update(nul)
        return lib.raw("mvs_bn_bwd_reduce_slots", p(a["dy"]), p(a["x"]), p(a["stats"]), 1, G, Vg, C, p(a["slots"]), ns, s)

    def bwd(C=C, G=1, ns=ns, **nul):
        a = dict(dy=x, x=x, stats=stats, slots=slots, dx=dx)
        a.update(nul)
        return lib.raw("mvs_bn_relu_bwd_slots", p(a["dy"]), p(a["x"]), p(a["stats"]), p(a["slots"]), ns, 1, G, Vg, C, p(a["dx"]), p(v), p(v), s)

    for f in (stats_slots, fwd, fin, red, bwd):
        assert f(C=12) != 0, f.__name__ + ": C = 12"
        for bad in (3, 512, 0):
            assert f(ns=bad) != 0, "%s: nslots = %d" % (f.__name__, bad)
        for bad in (0, 65):
            assert f(G=bad) != 0, "%s: G = %d" % (f.__name__, bad)
    assert lib.raw("mvs_bn_relu_fwd", p(x), p(v), p(v), None, 1, Vg, 12, p(y), s) != 0
    for f in (fwd, fin):
        assert f(rv=None) != 0 and f(rm=None) != 0, f.__name__ + ": running_mean without running_var"
    assert stats_slots(x_=None) != 0 and stats_slots(slots_=None) != 0
    for f, names in ((fwd, ("x", "slots", "gamma", "beta", "stats", "y")), (fin, ("slots", "gamma", "beta", "stats")),
                     (red, ("dy", "x", "stats", "slots")), (bwd, ("dy", "x", "stats", "slots", "dx"))):
        for n in names:
            assert f(**{n: None}) != 0, "%s: %s = NULL" % (f.__name__, n)
    for i in range(6):
        a = [p(v)] * 6
        a[i] = None
        assert lib.raw("mvs_bn_eval_affine", a[0], a[1], a[2], a[3], EPS, C, a[4], a[5], s) != 0
    for i in (0, 1, 2, 4):
        a = [p(x), p(v), p(v), None, p(y)]
        a[i] = None
        assert lib.raw("mvs_bn_relu_fwd", a[0], a[1], a[2], a[3], 1, Vg, C, a[4], s) != 0
    assert lib.launch_trace() == [], "a rejected call launched a kernel"
    assert fwd(rm=torch.zeros(C, device=dev), rv=torch.ones(C, device=dev)) == 0 and lib.launch_trace() == ["bn_relu_fwd_slots"]       # (the good call does launch: the trace is live)
    if dev.type == "cuda":
        torch.cuda.synchronize()


SWEEP_RATIOS = (0, 1, 4, 32)
SWEEP_SHAPES = ((8, 4096), (32, 105))


def conditioning_case(dev, C, rows, ratio):
    """case 9: channel mean / std = ratio, relu off; every tensor as accurate as max(A, B) allows (see the module docstring).
    With one fp32 chain over a workgroup's 256 partial sums (bn_block_to_slot before it summed them in fp64) C = 8 x 4096 rows at ratio
    32 missed this on running_var, in the emulation and on the device alike: 9.97e-6 against B's 1.82e-6 and A's 8.2e-8; now 1.6e-7.
    The measured table is in DESIGN.md ("Conditioning of the train-mode statistics")."""
    inp = inputs(C, rows, 1, ratio)
    ours = run_kernels(dev, inp, 0, False, dims=DIMS[rows])
    compare(Record("conditioning C=%d rows=%d mean/std=%d" % (C, rows, ratio), dev), inp, ours, 0, False, sweep=True)
