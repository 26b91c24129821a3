"""The stage glue of a CVPMVSNet forward on HIP (csrc/cvp_stage_kernels.h: mvs_cvp_cameras, mvs_depth_hypo_up; ops.cvp_cameras,
ops.depth_hypotheses_up; CVPMVSNet.hip_stage): the cases shared by tests/test_cvp_stage.py (CPU emulation of the kernel sources) and
tests/test_gpu_cvp_stage.py (the same cases on the device).  Every case takes the device.

Truth for the cameras is exact rational arithmetic (fractions.Fraction) from the fp32 inputs; every product reads the conditioned
intrinsics as rounded to fp32 -- what in_ms holds and what the reference's lines read.  Truth for the level transition is the fp64
bilinear restatement below and oracle.ref_torch.cal_depth_hypo applied to it; the yardstick is today's path on the same device.
Measured ratios go to cvp_stage_parity_ratios.jsonl next to the file MVS_GRAD_REPORT names; the GPU run's copy kept with the project
is profiles/cvp_stage_parity_ratios.jsonl."""
import ctypes as C
import json
import math
import os
import re
import types
from fractions import Fraction

import numpy as np
import torch
import torch.nn.functional as F

from conftest import load_golden, rel_l1, state_dict_from
from oracle import ref_torch as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = 1024                       # canary elements behind every exactly-sized buffer a kernel writes
# fine sizes of the level transition: every clamp; one partial workgroup with all four borders; exactly two workgroups; three
# workgroups, the last partial (a workgroup is 256 fine pixels)
UP_SHAPES = ((2, 2), (6, 10), (16, 32), (18, 34))
# (B, S, L, image height, level heights): the smallest; two of each; the recipe's view count; the limits' side (10 views, 5 levels); and
# ratios that are no powers of two (150 / 75 = 2, 150 / 37 = 4.054...)
CAMERA_CASES = ((1, 1, 1, 64, (64,)), (2, 2, 2, 64, (64, 32)), (2, 6, 2, 128, (128, 64)), (1, 10, 5, 160, (160, 80, 40, 20, 10)),
                (2, 3, 3, 150, (150, 75, 37)))
NEW_LABELS = ("cvp_cameras", "depth_hypo_up_interval", "depth_hypo_up_write")


def _dev_lib(dev):
    from mvs_amd import _lib
    lib = _lib.get()
    assert lib.device_type == dev.type, "the library serves %s tensors, the case runs on %s" % (lib.device_type, dev)
    return lib


def _stream(t):
    from mvs_amd import ops
    return ops._stream(t)


def _owned(n, dev, dtype=torch.float32):
    """an output buffer of exactly n elements, NaN-filled, with TAIL canary elements behind it (the conv2d_arm_cases.py idiom)"""
    buf = torch.full((n + TAIL,), float("nan"), dtype=dtype, device=dev)
    buf[n:] = 12345.0
    return buf


def _check_owned(buf, n, what):
    assert bool((buf[n:] == 12345.0).all()), "%s: wrote behind its %d elements" % (what, n)
    assert not bool(torch.isnan(buf[:n]).any()), "%s: left output elements unwritten" % what
    return buf[:n]


def _record(rows):
    out_dir = os.path.dirname(os.path.abspath(os.environ["MVS_GRAD_REPORT"])) if os.environ.get("MVS_GRAD_REPORT") else ""
    if not out_dir:
        return
    try:
        with open(os.path.join(out_dir, "cvp_stage_parity_ratios.jsonl"), "a") as fh:
            for row in rows:
                fh.write(json.dumps(row) + "\n")
    except OSError:
        pass


def ulp32(x):
    """the spacing of fp32 numbers at magnitude x"""
    x = abs(float(x))
    return 2.0 ** -149 if x < 2.0 ** -126 else 2.0 ** (math.floor(math.log2(x)) - 23)


# ------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------
def camera_inputs(B, S, img_h, img_w):
    """synthetic.synthetic_cameras at the image size, different per batch item (focal length, principal point, baselines, range)"""
    K, E = R.synthetic_cameras(S + 1, img_h, img_w, img_w)
    ref_in, src_in = K.unsqueeze(0).repeat(B, 1, 1), K.view(1, 1, 3, 3).repeat(B, S, 1, 1)
    ref_ex, src_ex = E[0].unsqueeze(0).repeat(B, 1, 1), E[1:].unsqueeze(0).repeat(B, 1, 1, 1).clone()
    for b in range(1, B):
        ref_in[b, :2, :2] *= 1.0 + 0.03 * b
        src_in[b, :, :2, :2] *= 1.0 - 0.02 * b
        src_in[b, :, :2, 2] += 0.37 * b
        src_ex[b, :, :3, 3] *= 1.0 + 0.4 * b
    dmin = torch.tensor([425.0 + 3.3 * b for b in range(B)])
    dmax = torch.tensor([425.0 + 47 * 13.5 + 1.7 * b for b in range(B)])
    return ref_in, src_in, ref_ex, src_ex, dmin, dmax


def fixture_cameras(name):
    """the cameras the g7 fixture carries, and the ones the g13 fixture was made with (tests/test_oracle_vs_reference.py)"""
    if name == "g7":
        g = load_golden("g7_cvpmvsnet_e2e")
        return tuple(g[k] for k in ("ref_in", "src_in", "ref_ex", "src_ex", "depth_min", "depth_max")) + (64, (64, 32))
    load_golden("g13_cvpmvsnet_three_levels_a")
    K, E = R.synthetic_cameras(4, 96, 128, 128)
    return (K.unsqueeze(0), K.view(1, 1, 3, 3).repeat(1, 3, 1, 1), E[0].unsqueeze(0), E[1:].unsqueeze(0), torch.tensor([425.0]),
            torch.tensor([425.0 + 47 * 13.5]), 96, (96, 48, 24))


def host_mats(ki, ks, ei, es):
    """today's host lines of calDepthHypo (jdacs_ms/models/modules.py:72-80) on the CPU: [B,30] fp64 from the level's fp32
    intrinsics ki / ks [B,3,3] (source view 0) and the extrinsics ei / es [B,4,4]"""
    ki, ks, ei, es = ki.double().cpu(), ks.double().cpu(), ei.double().cpu(), es.double().cpu()
    inv = lambda m: torch.linalg.inv_ex(m).inverse
    T = ks @ (es @ inv(ei))[:, :3, :]
    A = (ki @ ei[:, :3, :3]) @ inv(ks @ es[:, :3, :3])
    nb = ki.shape[0]
    return torch.cat([inv(ki).reshape(nb, 9), T.reshape(nb, 12), A.reshape(nb, 9)], 1)


def up_inputs(H, W):
    """B = 2: item 0 looks at synthetic view 1, item 1 at view 2; coarse depths are smooth ramps around 500-800 with per-pixel noise"""
    h, w = H // 2, W // 2
    K, E = R.synthetic_cameras(3, H, W, 4 * W)
    ki, ks = K.unsqueeze(0).repeat(2, 1, 1), K.unsqueeze(0).repeat(2, 1, 1)
    ei, es = E[0].unsqueeze(0).repeat(2, 1, 1), E[1:3].clone()
    gen = torch.Generator().manual_seed(100 * H + W)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    depth = torch.stack([560.0 + 90.0 * xx / w + 50.0 * yy / h, 760.0 - 70.0 * xx / w + 30.0 * yy / h]) + 6.0 * torch.rand(2, h, w, generator=gen)
    return depth.contiguous(), host_mats(ki, ks, ei, es), (ki, ks.unsqueeze(1), ei, es.unsqueeze(1))


# ------------------------------------------------------------------------------------------------------------------------
# fp64 restatements
# ------------------------------------------------------------------------------------------------------------------------
def up64(d):
    """x2 bilinear up-sampling of [B,h,w] in fp64, F.interpolate(scale_factor=2, align_corners=None) written out: src = (dst + 0.5) / 2
    - 0.5 clamped at 0, the upper neighbour clamped at the last row / column"""
    d = d.double()
    _, h, w = d.shape

    def axis(n):
        src = ((torch.arange(2 * n, dtype=torch.float64) + 0.5) / 2 - 0.5).clamp_min(0)
        i0 = src.floor().long()
        return i0, (i0 + 1).clamp_max(n - 1), src - i0
    y0, y1, ly = axis(h)
    x0, x1, lx = axis(w)
    top = d[:, y0][:, :, x0] * (1 - lx) + d[:, y0][:, :, x1] * lx
    bot = d[:, y1][:, :, x0] * (1 - lx) + d[:, y1][:, :, x1] * lx
    out = top * (1 - ly)[None, :, None] + bot * ly[None, :, None]
    assert float((out - F.interpolate(d[None], scale_factor=2, mode="bilinear", align_corners=None)[0]).abs().max()) <= 1e-9
    return out


def interval64(up, mats):
    """per fine pixel, in fp64 from the [B,30] matrices: the determinant of calDepthHypo's 2x2 system and the interval magnitude"""
    B, H, W = up.shape
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    X = torch.stack([xx, yy, torch.ones_like(xx)], 0).reshape(3, -1)
    dets, mags = [], []
    for b in range(B):
        Ki, T, A = mats[b, :9].view(3, 3), mats[b, 9:21].view(3, 4), mats[b, 21:].view(3, 3)

        def to_src(dz):
            pix = T[:, :3] @ ((Ki @ X) * dz) + T[:, 3:]
            return pix / pix[2:], pix[2]
        d1 = up[b].double().reshape(-1)
        X1, z1 = to_src(d1)
        X2, _ = to_src(d1 + 1)
        theta = torch.atan((X2[1] - X1[1]) / (X2[0] - X1[0]))
        X3 = X1 + torch.stack([torch.cos(theta), torch.sin(theta), torch.zeros_like(theta)])
        t1, t2 = z1 * (A @ X1), A @ X3
        det = X[1] * t2[2] - t2[1]
        dets.append(det)
        mags.append(((t2[2] * t1[1] - t2[1] * t1[2]) / det).abs())
    return torch.stack(dets), torch.stack(mags)


def assert_well_conditioned(up, mats, what):
    """the precondition of every level-transition case, on the fp64 restatement: min|det| >= 0.25 median|det|, max interval <= 4 median"""
    det, mag = interval64(up, mats)
    assert bool(torch.isfinite(det).all()) and bool(torch.isfinite(mag).all()), what
    for b in range(det.shape[0]):
        d, m = det[b].abs(), mag[b]
        assert float(d.min()) >= 0.25 * float(d.median()), "%s item %d: min|det| %.3e, median %.3e" % (what, b, float(d.min()), float(d.median()))
        assert float(m.max()) <= 4.0 * float(m.median()), "%s item %d: max interval %.3e, median %.3e" % (what, b, float(m.max()), float(m.median()))


# ------------------------------------------------------------------------------------------------------------------------
# 1. the level transition
# ------------------------------------------------------------------------------------------------------------------------
def raw_up(lib, dev, depth_d, mats_d, want_up=True):
    """mvs_depth_hypo_up into exactly sized buffers with canaries behind them -> (hypos [B,8,2h,2w], depth_up [B,2h,2w] or None)"""
    B, h, w = depth_d.shape
    nws = int(lib.raw("mvs_depth_hypo_workspace_doubles", B, 2 * h, 2 * w))
    assert nws == B * ((4 * h * w + 255) // 256)
    ws, hyp = _owned(nws, dev, torch.float64), _owned(B * 8 * 4 * h * w, dev)
    up = _owned(B * 4 * h * w, dev) if want_up else None
    lib.launch_trace()
    lib.call("mvs_depth_hypo_up", depth_d.data_ptr(), mats_d.data_ptr(), B, h, w, ws.data_ptr(), hyp.data_ptr(),
             None if up is None else up.data_ptr(), _stream(depth_d))
    assert lib.launch_trace() == ["depth_hypo_up_interval", "depth_hypo_up_write"]
    _check_owned(ws, nws, "depth_hypo_up workspace")
    hyp = _check_owned(hyp, B * 8 * 4 * h * w, "depth_hypo_up hypos").view(B, 8, 2 * h, 2 * w)
    return hyp, None if up is None else _check_owned(up, B * 4 * h * w, "depth_hypo_up depth_up").view(B, 2 * h, 2 * w)


def up_case(dev, H, W):
    """depth_up within 4 ulp_fp32(max|d|) of the fp64 restatement (the products by 0.25 / 0.75 and the three sums round at most once
    each, by half an ulp of a value no larger than max|d|); hypos against the oracle on the fp64 up-sampled depth: at most 2 x the
    error of today's path (F.interpolate + ops.depth_hypotheses on the same device) + 1 ulp_fp32(max|d|) -- both round the same
    quantities to fp32 once and differ in summation order only; two calls and the call without depth_up give the same bits."""
    from mvs_amd import ops
    lib = _dev_lib(dev)
    depth, mats, cams = up_inputs(H, W)
    truth_up = up64(depth)
    assert_well_conditioned(truth_up, mats, "fine %dx%d" % (H, W))
    depth_d, mats_d = depth.to(dev), mats.to(dev)
    hyp, up = raw_up(lib, dev, depth_d, mats_d)
    u = ulp32(depth.abs().max())
    e_up = float((up.cpu().double() - truth_up).abs().max())
    print("depth_hypo_up %dx%d: depth_up max err %.3e = %.2f ulp (bound 4)" % (H, W, e_up, e_up / u))
    assert e_up <= 4 * u
    want = R.cal_depth_hypo(truth_up, cams[0], cams[1], cams[2], cams[3]).double()
    today_up = F.interpolate(depth_d[None, :], size=None, scale_factor=2, mode="bilinear", align_corners=None).squeeze(0)
    today = ops.depth_hypotheses(today_up, mats_d)
    e_new, e_today = float((hyp.cpu().double() - want).abs().max()), float((today.cpu().double() - want).abs().max())
    print("depth_hypo_up %dx%d: hypos max err %.3e, today's path %.3e, ulp %.3e" % (H, W, e_new, e_today, u))
    _record([{"what": "depth_hypo_up hypos vs oracle", "device": str(dev), "fine": [H, W], "new_err": e_new, "today_err": e_today,
              "ratio": e_new / max(e_today, 1e-300), "depth_up_err_ulp": e_up / u, "ulp": u}])
    assert e_new <= 2 * e_today + u, "hypos: %.3e above 2 x %.3e + %.3e" % (e_new, e_today, u)
    # determinism, the null depth_up pointer, the wrapper
    hyp2, up2 = raw_up(lib, dev, depth_d, mats_d)
    assert torch.equal(hyp, hyp2) and torch.equal(up, up2)
    hyp3, none = raw_up(lib, dev, depth_d, mats_d, want_up=False)
    assert none is None and torch.equal(hyp, hyp3)
    o_h, o_u = ops.depth_hypotheses_up(depth_d, mats_d, want_depth_up=True)
    assert torch.equal(o_h, hyp) and torch.equal(o_u, up) and torch.equal(ops.depth_hypotheses_up(depth_d, mats_d), hyp)


def up_fixture_case(dev):
    """g7's coarse depth map (32x48) through the transition: depth_up and hypos0 of the fixture within the 1e-3 that
    test_emul_kernels.py / test_gpu_parity.py allow calDepthHypo on this fixture"""
    from mvs_amd import ops
    _dev_lib(dev)
    g = load_golden("g7_cvpmvsnet_e2e")
    mats = host_mats(g["ref_in"], g["src_in"][:, 0], g["ref_ex"], g["src_ex"][:, 0])
    hyp, up = ops.depth_hypotheses_up(g["depth1"].to(dev), mats.to(dev), want_depth_up=True)
    assert hyp.shape == g["hypos0"].shape and hyp.dtype == torch.float32 and up.shape == g["depth_up"].shape
    e_u, e_h = float((up.cpu() - g["depth_up"]).abs().max()), float((hyp.cpu() - g["hypos0"]).abs().max())
    print("g7 through depth_hypo_up: depth_up err %.3e, hypos0 err %.3e" % (e_u, e_h))
    assert e_u < 1e-3 and e_h < 1e-3


def up_refuse_case(dev):
    lib = _dev_lib(dev)
    lib.launch_trace()
    t = torch.zeros(64, dtype=torch.float64, device=dev)
    p = t.data_ptr()
    assert lib.raw("mvs_depth_hypo_up", None, p, 1, 2, 2, p, p, None, None) == -4
    assert lib.raw("mvs_depth_hypo_up", p, p, 1, 2, 2, p, None, None, None) == -4
    assert lib.raw("mvs_depth_hypo_up", p, p, 0, 2, 2, p, p, None, None) == -1
    assert lib.raw("mvs_depth_hypo_up", p, p, 1, 0, 2, p, p, None, None) == -1
    assert lib.launch_trace() == []


# ------------------------------------------------------------------------------------------------------------------------
# 2. the cameras
# ------------------------------------------------------------------------------------------------------------------------
def _fr(t):
    """a float tensor as nested lists of exact Fractions"""
    a = t.detach().cpu().double().numpy()
    return np.vectorize(Fraction, otypes=[object])(a)


def _inverse(m):
    """exact inverse of a square object array of Fractions (Gauss-Jordan)"""
    n = m.shape[0]
    a = [[m[r][c] for c in range(n)] + [Fraction(int(r == c)) for c in range(n)] for r in range(n)]
    for col in range(n):
        piv = next(r for r in range(col, n) if a[r][col] != 0)
        a[col], a[piv] = a[piv], a[col]
        s = a[col][col]
        a[col] = [v / s for v in a[col]]
        for r in range(n):
            if r != col and a[r][col] != 0:
                f = a[r][col]
                a[r] = [v - f * p for v, p in zip(a[r], a[col])]
    return np.array([row[n:] for row in a], dtype=object)


def _round32(q):
    """a Fraction rounded to fp64 (correctly), then to fp32: how the kernel rounds a conditioned intrinsic"""
    return float(np.float32(float(q)))


def _err(out, exact):
    """element-wise |out - exact| as floats; out: float array, exact: object array of Fractions of the same shape"""
    o = np.vectorize(Fraction, otypes=[object])(np.asarray(out, dtype=np.float64))
    return np.vectorize(lambda a, b: float(abs(a - b)), otypes=[np.float64])(o, exact)


def _mag(exact):
    return np.vectorize(lambda a: float(abs(a)), otypes=[np.float64])(exact)


def exact_cameras(ref_in, src_in, ref_ex, src_ex, dmin, dmax, img_h, level_hs):
    """Exact rational results from the fp32 inputs.  Returns the exact conditioned intrinsics q [B,S+1,L,3,3], their fp32 roundings k32
    (what every product below reads), proj [L][B][S] (3x4 exact), mats [L-1][B] (30 exact), planes (48 exact)."""
    B, S, L = ref_in.shape[0], src_in.shape[1], len(level_hs)
    Ks = np.concatenate([_fr(ref_in)[:, None], _fr(src_in)], 1)           # [B,S+1,3,3]
    Es = np.concatenate([_fr(ref_ex)[:, None], _fr(src_ex)], 1)           # [B,S+1,4,4]
    q = np.empty((B, S + 1, L, 3, 3), dtype=object)
    for l, lh in enumerate(level_hs):
        q[:, :, l] = Ks
        q[:, :, l, :2, :] = Ks[:, :, :2, :] * Fraction(lh, img_h)
    k32 = np.vectorize(_round32, otypes=[np.float64])(q)
    kx = np.vectorize(Fraction, otypes=[object])(k32)
    last = np.array([[Fraction(0), Fraction(0), Fraction(0), Fraction(1)]], dtype=object)
    proj, mats = [], []
    for l in range(L):
        pl, ml = [], []
        for b in range(B):
            P = [np.concatenate([kx[b, v, l].dot(Es[b, v][:3, :]), last], 0) for v in range(S + 1)]
            Pi = _inverse(P[0])
            pl.append([P[v].dot(Pi)[:3, :] for v in range(1, S + 1)])
            if l < L - 1:
                ki, ks, ei, es = kx[b, 0, l], kx[b, 1, l], Es[b, 0], Es[b, 1]
                T = ks.dot(es.dot(_inverse(ei))[:3, :])
                A = ki.dot(ei[:3, :3]).dot(_inverse(ks.dot(es[:3, :3])))
                ml.append(np.concatenate([_inverse(ki).reshape(-1), T.reshape(-1), A.reshape(-1)]))
        proj.append(pl)
        mats.append(ml)
    d0, d1 = Fraction(float(dmin[0])), Fraction(float(dmax[0]))
    planes = np.array([d0 + i * (d1 - d0) / 47 for i in range(48)], dtype=object)
    return q, k32, proj, mats[:L - 1], planes


def raw_cameras(lib, dev, ins, img_h, level_hs, mats_canary=False):
    """mvs_cvp_cameras into exactly sized buffers with canaries behind them"""
    ref_in, src_in, ref_ex, src_ex, dmin, dmax = [t.to(dev).float().contiguous() for t in ins]
    B, S, L = ref_in.shape[0], src_in.shape[1], len(level_hs)
    sizes = {"in_ms": B * (S + 1) * L * 9, "rot": L * B * S * 9, "trans": L * B * S * 3, "planes": B * 48}
    bufs = {k: _owned(n, dev) for k, n in sizes.items()}
    nm = (L - 1) * B * 30
    mats = _owned(nm, dev, torch.float64)
    lib.launch_trace()
    lib.call("mvs_cvp_cameras", ref_in.data_ptr(), src_in.data_ptr(), ref_ex.data_ptr(), src_ex.data_ptr(), dmin.data_ptr(), dmax.data_ptr(),
             B, S, L, img_h, (C.c_int * L)(*level_hs), bufs["in_ms"].data_ptr(), bufs["rot"].data_ptr(), bufs["trans"].data_ptr(),
             mats.data_ptr() if (L > 1 or mats_canary) else None, bufs["planes"].data_ptr(), _stream(ref_in))
    assert lib.launch_trace() == ["cvp_cameras"]                     # everything in ONE launch
    out = {k: _check_owned(bufs[k], n, "cvp_cameras " + k) for k, n in sizes.items()}
    if L > 1:
        out["mats"] = _check_owned(mats, nm, "cvp_cameras mats").view(L - 1, B, 30)
    else:
        assert bool((mats == 12345.0).all()), "cvp_cameras with one level wrote matrices"
    return (out["in_ms"].view(B, S + 1, L, 3, 3), out["rot"].view(L, B, S, 3, 3), out["trans"].view(L, B, S, 3), out.get("mats"),
            out["planes"].view(B, 48))


def cameras_case(dev, ins, img_h, level_hs, what):
    from mvs_amd import ops
    from mvs_amd.jdacs_ms.models import modules as M
    lib = _dev_lib(dev)
    ref_in, src_in, ref_ex, src_ex, dmin, dmax = ins
    B, S, L = ref_in.shape[0], src_in.shape[1], len(level_hs)
    in_ms, rot, trans, mats, planes = raw_cameras(lib, dev, ins, img_h, level_hs, mats_canary=True)
    q, k32, proj, xmats, xplanes = exact_cameras(ref_in, src_in, ref_ex, src_ex, dmin, dmax, img_h, level_hs)
    rows = []
    # in_ms: at most 1 ulp from the exact value; the bits of conditionIntrinsics where every ratio is a power of two
    got = in_ms.cpu().double().numpy()
    e = _err(got, q)
    assert all(e[i] <= ulp32(_mag(q)[i]) for i in np.ndindex(*e.shape)), "%s: in_ms more than 1 ulp from the exact value" % what
    assert np.array_equal(got, k32), "%s: in_ms is not the exact value rounded to fp64, then fp32" % what
    fp_shapes = [(B, 16, lh, 1) for lh in level_hs]
    today_ms = torch.stack([M.conditionIntrinsics(k, (B, 3, img_h, 1), fp_shapes)
                            for k in [ref_in] + [src_in[:, s] for s in range(S)]], 1)
    if all(img_h % lh == 0 and (img_h // lh) & (img_h // lh - 1) == 0 for lh in level_hs):
        assert torch.equal(in_ms.cpu(), today_ms), "%s: in_ms differs from conditionIntrinsics" % what
    # rot / trans: within 1 ulp_fp32 of the row's largest magnitude, and never above today's _ms_proj + relative_projections
    today_d = today_ms.to(dev)
    for l in range(L):
        with torch.no_grad():
            t_rot, t_trans = ops.relative_projections([M._ms_proj(today_d[:, s + 1, l], src_ex[:, s].to(dev)) for s in range(S)],
                                                      M._ms_proj(today_d[:, 0, l], ref_ex.to(dev)))
        new = torch.cat([rot[l], trans[l].unsqueeze(-1)], -1).cpu().double().numpy()          # [B,S,3,4]
        old = torch.cat([t_rot, t_trans.unsqueeze(-1)], -1).cpu().double().numpy()
        exact = np.array(proj[l], dtype=object)
        e_new, e_old, mag = _err(new, exact), _err(old, exact), _mag(exact)
        worst = 0.0
        for b in range(B):
            for s in range(S):
                for r in range(3):
                    u = ulp32(mag[b, s, r].max())
                    worst = max(worst, e_new[b, s, r].max() / u)
                    assert e_new[b, s, r].max() <= u, "%s level %d item %d view %d row %d: %.3e above 1 ulp %.3e" % (what, l, b, s, r, e_new[b, s, r].max(), u)
        rows.append({"what": "cvp_cameras rot/trans vs exact", "case": what, "device": str(dev), "level": l, "new_err": float(e_new.max()),
                     "today_err": float(e_old.max()), "ratio": float(e_new.max()) / max(float(e_old.max()), 1e-300), "worst_row_ulp": worst})
        print("%s level %d: rot/trans max err %.3e (%.2f ulp of its row), today's path %.3e" % (what, l, e_new.max(), worst, e_old.max()))
        assert e_new.max() <= e_old.max(), "%s level %d: %.3e above today's %.3e" % (what, l, e_new.max(), e_old.max())
    # mats: per block at most 4 x the error of today's torch fp64 lines on the CPU (floor: 64 * 2^-53 of the block's largest magnitude)
    for l in range(L - 1):
        k_l = torch.from_numpy(k32[:, :, l]).float()
        old = host_mats(k_l[:, 0], k_l[:, 1], ref_ex, src_ex[:, 0]).numpy()
        new = mats[l].cpu().numpy()
        exact = np.array(xmats[l], dtype=object)
        for name, (lo, hi) in (("Kinv", (0, 9)), ("T", (9, 21)), ("A", (21, 30))):
            e_new, e_old = _err(new[:, lo:hi], exact[:, lo:hi]).max(), _err(old[:, lo:hi], exact[:, lo:hi]).max()
            floor = 64 * 2.0 ** -53 * _mag(exact[:, lo:hi]).max()
            rows.append({"what": "cvp_cameras mats vs exact", "case": what, "device": str(dev), "level": l, "block": name, "new_err": float(e_new),
                         "today_err": float(e_old), "ratio": float(e_new) / max(float(e_old), 1e-300), "floor": floor})
            print("%s level %d mats %s: err %.3e, torch fp64 on the CPU %.3e, floor %.3e" % (what, l, name, e_new, e_old, floor))
            assert e_new <= max(4 * e_old, floor), "%s level %d block %s: %.3e above max(4 x %.3e, %.3e)" % (what, l, name, e_new, e_old, floor)
    # planes: within 1 ulp of the exact value rounded to fp32; every item gets item 0's; at most 4 ulp_fp32(depth_max) from today's
    pl = planes.cpu().double().numpy()
    assert all(np.array_equal(pl[b], pl[0]) for b in range(B))
    for i in range(48):
        r = _round32(xplanes[i])
        assert abs(pl[0, i] - r) <= ulp32(r), "%s plane %d: %.9g, exact %.9g" % (what, i, pl[0, i], r)
    today_pl = M.calSweepingDepthHypo(ref_in, src_in[:, 0], ref_ex, src_ex, dmin, dmax)
    dist = float((planes.cpu() - today_pl).abs().max())
    rows.append({"what": "cvp_cameras planes vs calSweepingDepthHypo", "case": what, "device": str(dev), "distance": dist,
                 "ulp_of_depth_max": ulp32(dmax[0])})
    assert dist <= 4 * ulp32(dmax[0])
    _record(rows)
    # the wrapper: same bits, also from float64 cameras that live on the CPU
    outs = ops.cvp_cameras(ref_in.double(), src_in.double(), ref_ex.double(), src_ex.double(), dmin.double(), dmax.double(), img_h,
                           level_hs, like=in_ms)
    for a, b_ in zip(outs, (in_ms, rot, trans, mats, planes)):
        assert (b_ is None and a.numel() == 0) or torch.equal(a, b_)
    assert outs[3].dtype == torch.float64 and tuple(outs[3].shape) == (L - 1, B, 30)


def cameras_refuse_case(dev):
    """S = 11 or more levels than the limit: MVS_ERR_SHAPE; null pointers: MVS_ERR_NULL; nothing launched.  The wrapper raises."""
    import pytest
    from mvs_amd import ops
    lib = _dev_lib(dev)
    t = torch.zeros(4096, dtype=torch.float64, device=dev)
    p = t.data_ptr()
    lv = (C.c_int * 8)(*([8] * 8))
    lib.launch_trace()
    call = lambda *a: lib.raw("mvs_cvp_cameras", *a)
    assert call(p, p, p, p, p, p, 1, 11, 2, 8, lv, p, p, p, p, p, None) == -1
    assert call(p, p, p, p, p, p, 1, 0, 2, 8, lv, p, p, p, p, p, None) == -1
    assert call(p, p, p, p, p, p, 1, 2, ops.PYRAMID_MAX_LEVELS + 1, 8, lv, p, p, p, p, p, None) == -1
    assert call(p, p, p, p, p, p, 1, 2, 0, 8, lv, p, p, p, p, p, None) == -1
    assert call(p, p, p, p, p, p, 1, 2, 2, 8, (C.c_int * 2)(8, 0), p, p, p, p, p, None) == -1
    assert call(None, p, p, p, p, p, 1, 2, 2, 8, lv, p, p, p, p, p, None) == -4
    assert call(p, p, p, p, p, p, 1, 2, 2, 8, lv, p, p, p, None, p, None) == -4          # two levels need the matrices
    assert call(p, p, p, p, p, p, 1, 2, 2, 8, lv, p, p, None, p, p, None) == -4
    assert call(p, p, p, p, p, p, 1, 2, 2, 8, None, p, p, p, p, p, None) == -4
    assert lib.launch_trace() == []
    ins = camera_inputs(1, 11, 64, 96)
    with pytest.raises(ValueError, match="source views"):
        ops.cvp_cameras(*[x.to(dev) for x in ins], 64, (64, 32))
    ins = camera_inputs(1, 2, 64, 96)
    with pytest.raises(ValueError, match="levels"):
        ops.cvp_cameras(*[x.to(dev) for x in ins], 64, (64,) * (ops.PYRAMID_MAX_LEVELS + 1))
    if dev.type == "cuda":               # CPU tensors and no `like`: no host restatement, the error calDepthHypo raises today
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.cvp_cameras(*ins, 64, (64, 32))


# ------------------------------------------------------------------------------------------------------------------------
# 3. the model
# ------------------------------------------------------------------------------------------------------------------------
def _glue_trace(lib, net, ins):
    """the launch labels of one forward outside the feature pyramid and the regulariser (the library keeps the first 64 labels of a
    read, a whole forward has more: the modules' hooks read in between)"""
    glue = []

    def drop(*_):
        lib.launch_trace()

    def keep(*_):
        glue.extend(lib.launch_trace())
    hooks = [net.featurePyramid.register_forward_hook(drop), net.cost_reg_refine.register_forward_pre_hook(keep),
             net.cost_reg_refine.register_forward_hook(drop)]
    try:
        lib.launch_trace()
        with torch.no_grad():
            out = net(*ins)
        glue.extend(lib.launch_trace())
    finally:
        for h in hooks:
            h.remove()
    return glue, out


def model_inputs(dev, B, nsrc, H, W, seed=3):
    gen = torch.Generator().manual_seed(seed)
    ref_in, src_in, ref_ex, src_ex, dmin, dmax = camera_inputs(B, nsrc, H, W)
    ins = [F.avg_pool2d(torch.randn(B, 3, H, W, generator=gen), 5, 1, 2), F.avg_pool2d(torch.randn(B * nsrc, 3, H, W, generator=gen), 5, 1, 2).view(B, nsrc, 3, H, W),
           ref_in, src_in, ref_ex, src_ex, dmin, dmax]
    return [t.to(dev) for t in ins]


class _ChannelMean(torch.nn.Module):
    """stands in for the regulariser where its emulation would take minutes: the stage glue under test neither runs nor reads it"""

    def forward(self, x):
        return x.mean(1) * 50.0


def launch_trace_case(dev, H=32, W=48, nscale=2, stub_regulariser=False):
    """one forward (B = 1, nsrc = 2) with the stage on: exactly one cvp_cameras and, per refine level, one depth_hypo_up_interval + one
    depth_hypo_up_write, no relative_projection and no depth_hypo launch; with it off: today's labels and none of the three new ones.
    The class default follows MVS_HIP_CVP_STAGE; cameras on the CPU next to device features give the same bits."""
    from mvs_amd.jdacs_ms.models.network import CVPMVSNet
    lib = _dev_lib(dev)
    assert CVPMVSNet.hip_stage == (os.environ.get("MVS_HIP_CVP_STAGE", "1") == "1")
    torch.manual_seed(0)
    net = CVPMVSNet(R.cvp_args(nsrc=2, nscale=nscale, mode="train"))
    if stub_regulariser:
        net.cost_reg_refine = _ChannelMean()
    net = net.to(dev).train()
    ins = model_inputs(dev, 1, 2, H, W)
    net.hip_stage = True
    on, out_on = _glue_trace(lib, net, ins)
    assert on.count("cvp_cameras") == 1 and on[0] == "cvp_cameras", on
    assert on.count("depth_hypo_up_interval") == nscale - 1 and on.count("depth_hypo_up_write") == nscale - 1, on
    assert not any(lab in ("relative_projection", "depth_hypo", "depth_hypo_interval") for lab in on), on
    net.hip_stage = False
    off, out_off = _glue_trace(lib, net, ins)
    assert not any(lab in NEW_LABELS for lab in off), off
    assert off.count("relative_projection") == nscale and off.count("depth_hypo") == nscale - 1, off
    assert [lab for lab in on if lab not in NEW_LABELS] == [lab for lab in off if lab not in ("relative_projection", "depth_hypo")]
    off2, out_off2 = _glue_trace(lib, net, ins)
    assert off2 == off and all(torch.equal(a, b) for a, b in zip(out_off["depth_est_list"], out_off2["depth_est_list"]))
    # both paths evaluate the same geometry: the coarse level differs by the planes' and the projections' last bits only
    assert rel_l1(out_on["depth_est_list"][-1].cpu(), out_off["depth_est_list"][-1].cpu()) < 1e-4
    net.hip_stage = True
    if dev.type == "cpu":
        return net, ins
    cpu_cams = ins[:2] + [t.cpu() for t in ins[2:]]
    _, out_cpu = _glue_trace(lib, net, cpu_cams)
    assert all(torch.equal(a, b) for a, b in zip(out_on["depth_est_list"], out_cpu["depth_est_list"]))
    assert torch.equal(out_on["prob_confidence"], out_cpu["prob_confidence"])
    return net, ins


def g7_case(dev):
    """tests/test_gpu_parity.py::test_golden_cvpmvsnet_end_to_end with the stage on (and off, same weights): the fixture's depth maps
    within 1e-3 relative L1, its confidence within 5e-3 mean"""
    from mvs_amd.jdacs_ms.models.network import CVPMVSNet
    _dev_lib(dev)
    g = load_golden("g7_cvpmvsnet_e2e")
    net = CVPMVSNet(R.cvp_args(nsrc=2, nscale=2, mode="train"))
    net.load_state_dict(state_dict_from(g), strict=False)
    net = net.to(dev).train()
    ins = [g[k].to(dev) for k in ("ref_img", "src_imgs", "ref_in", "src_in", "ref_ex", "src_ex", "depth_min", "depth_max")]
    rows = []
    for stage in (True, False):
        net.hip_stage = stage
        with torch.no_grad():
            out = net(*ins)
        e1, e0 = rel_l1(out["depth_est_list"][1].cpu(), g["depth1"]), rel_l1(out["depth_est_list"][0].cpu(), g["depth0"])
        ec = float((out["prob_confidence"].cpu() - g["conf"]).abs().mean())
        print("g7 with hip_stage=%s: depth1 %.3e depth0 %.3e conf %.3e" % (stage, e1, e0, ec))
        rows.append({"what": "CVPMVSNet vs g7_cvpmvsnet_e2e", "device": str(dev), "hip_stage": stage, "depth1_rel_l1": e1, "depth0_rel_l1": e0,
                     "conf_mean_abs": ec})
        assert e1 < 1e-3 and e0 < 1e-3 and ec < 5e-3
    _record(rows)


def _rel(a, ref):
    ref = ref.double()
    return float((a.double().cpu() - ref).abs().sum()) / (float(ref.abs().sum()) + 1e-300)


def g13_case(dev):
    """tests/pyramid_cases.py::fixture_case with the stage on: per tensor (depth maps, confidence, the gradient of every parameter of the
    fixture's loss) the model's relative-L1 error against the g13 fixture is at most 4 x the error of R.OracleCVPMVSNet with stock ops on
    the same device, plus conftest's floors (2e-6 forward, 2e-5 gradients); the stage-off model under the same criterion next to it."""
    import copy
    from mvs_amd.jdacs_ms.models.network import CVPMVSNet
    _dev_lib(dev)
    g = {}
    for part in "abcd":
        g.update(load_golden("g13_cvpmvsnet_three_levels_" + part))
    torch.manual_seed(0)
    ora = R.OracleCVPMVSNet(types.SimpleNamespace(nsrc=3, nscale=3, mode="train"))
    for k, v in ora.state_dict().items():
        assert float(v.double().sum()) == float(g["sdsum." + k]), k
    gen = torch.Generator().manual_seed(2)
    ih, iw = 96, 128
    cams = fixture_cameras("g13")[:6]
    ins = [torch.randn(1, 3, ih, iw, generator=gen), torch.randn(1, 3, 3, ih, iw, generator=gen)] + list(cams)
    models = {"oracle": copy.deepcopy(ora)}
    for name, stage in (("stage_on", True), ("stage_off", False)):
        m = models[name] = CVPMVSNet(R.cvp_args(nsrc=3, nscale=3, mode="train"))
        m.load_state_dict(ora.state_dict())
        m.hip_stage = stage
    res = {}
    for name, model in models.items():
        model = model.to(dev).train()
        model.zero_grad(set_to_none=True)
        b = model(*[t.to(dev) for t in ins])
        sum(d.mean() for d in b["depth_est_list"]).backward()
        r = res[name] = {"depth_%d" % i: d.detach().cpu() for i, d in enumerate(b["depth_est_list"])}
        r["prob_confidence"] = b["prob_confidence"].detach().cpu()
        for k, q in model.named_parameters():
            if q.grad is not None and not k.endswith("prob0.bias"):
                r["grad." + k] = q.grad.detach().cpu()
    keys = sorted(res["stage_on"])
    assert set(keys) == set(res["oracle"]) == set(res["stage_off"]) and all(k in g for k in keys) and sum(k.startswith("grad.") for k in keys) >= 40
    rows, bad = [], []
    for k in keys:
        e_on, e_off, e_o = _rel(res["stage_on"][k], g[k]), _rel(res["stage_off"][k], g[k]), _rel(res["oracle"][k], g[k])
        floor = 2e-5 if k.startswith("grad.") else 2e-6
        rows.append({"what": "CVPMVSNet(hip_stage) vs g13_cvpmvsnet_three_levels", "device": str(dev), "tensor": k, "stage_on_err": e_on,
                     "stage_off_err": e_off, "oracle_err": e_o, "ratio": e_on / max(e_o, 1e-300), "slack_allowed": 4.0, "floor": floor})
        print("%-50s stage on %.3e off %.3e oracle %.3e" % (k, e_on, e_off, e_o))
        if e_on > 4.0 * e_o + floor:
            bad.append("%s: stage on %.3e vs oracle-on-device %.3e (stage off %.3e)" % (k, e_on, e_o, e_off))
    _record(rows)
    assert not bad, "less accurate than the oracle on the same device: " + "; ".join(bad)


def _kernel_names():
    """the names of this library's kernels, read from its sources"""
    names = set()
    csrc = os.path.join(ROOT, "self-supervised-mvs_amd", "csrc")
    for fn in os.listdir(csrc):
        if fn.endswith((".hip", ".h", ".cpp")):
            txt = open(os.path.join(csrc, fn)).read()
            names.update(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", txt))
    assert len(names) > 50 and "cvp_cameras_kernel" in names and "depth_hypo_up_write_kernel" in names
    return names


def _device_activities(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]


def profiler_case(dev):
    """GPU only: the device activities of one forward under torch.profiler with the stage off and on.  The foreign ones (not this
    library's kernels) with the stage on are a subset of those with it off and fewer; neither the kernel of F.interpolate(bilinear x2)
    nor any of torch.linalg.inv_ex on a [B,3,3] fp64 tensor (each profiled alone here) is among them."""
    net, ins = launch_trace_case(dev)
    ours = _kernel_names()
    mine = lambda n: any(k in ours for k in re.findall(r"\w+", n))
    # what a call profiled alone contributes: its own kernels, not the copies and the generic element-wise fills around them (a
    # forward zero-fills its BatchNorm slot arena, fp64, with the same FillFunctor<double> instantiation inv_ex uses for its identity)
    kernels = lambda names: {n for n in names if not n.startswith(("Memcpy", "Memset")) and "elementwise_kernel" not in n}

    def forward():          # autograd on: the feature pyramid takes its one-node pass, whose image pyramid is this library's kernel
        net(*ins)
    acts = {}
    for stage in (False, True):
        net.hip_stage = stage
        acts[stage] = _device_activities(forward)
    foreign = {s: [n for n in acts[s] if not mine(n)] for s in acts}
    d = torch.rand(1, 16, 24, device=dev) + 500.0
    m = torch.eye(3, dtype=torch.float64, device=dev).repeat(1, 1, 1) + 0.1 * torch.rand(1, 3, 3, dtype=torch.float64, device=dev)
    interp = kernels(_device_activities(lambda: F.interpolate(d[None, :], size=None, scale_factor=2, mode="bilinear", align_corners=None)))
    inv = kernels(_device_activities(lambda: torch.linalg.inv_ex(m).inverse))
    print("foreign device activities, stage off: %d %s" % (len(foreign[False]), sorted(set(foreign[False]))))
    print("foreign device activities, stage on: %d %s" % (len(foreign[True]), sorted(set(foreign[True]))))
    print("F.interpolate alone:", sorted(interp), "inv_ex alone:", sorted(inv))
    _record([{"what": "device activities of one CVPMVSNet forward (B=1, nsrc=2, 32x48, 2 levels)", "device": str(dev),
              "all_off": len(acts[False]), "all_on": len(acts[True]), "foreign_off": sorted(foreign[False]), "foreign_on": sorted(foreign[True]),
              "interpolate_alone": sorted(interp), "inv_ex_alone": sorted(inv)}])
    assert interp and inv and not any(mine(n) for n in interp | inv)
    assert any(n in interp for n in foreign[False]) and any(n in inv for n in foreign[False])
    assert set(foreign[True]) <= set(foreign[False]), sorted(set(foreign[True]) - set(foreign[False]))
    assert len(foreign[True]) < len(foreign[False])
    assert not [n for n in acts[True] if n in interp | inv], [n for n in acts[True] if n in interp | inv]
    assert sum("cvp_cameras_kernel" in n for n in acts[True]) == 1 and sum("depth_hypo_up_" in n for n in acts[True]) == 2
