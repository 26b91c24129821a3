#!/usr/bin/env python3
"""Timing evidence for SegDFF's feature extractor at the JDACS training shape (B = 1, N = 7, 3x512x640 images, the random
vgg19_trunk() weights of seed 0) on one GPU:
  (a) the stock path as SegDFF runs it without the HIP trunk: F.interpolate to 224x224 + net.features + permute / contiguous,
      with torch.backends.cudnn.benchmark off and on; the faster of the two is the row the decision uses;
  (b) the HIP path end to end: ops.resize_bilinear_cl + ops.conv_trunk_forward (weights packed once, outside the timing);
  (c) every layer of (b) on its own (mvs_conv2d_wide_fwd without the pool, mvs_maxpool2x2_cl): ms and the share of the
      157.3 TFLOP/s fp32 MFMA peak;
  (d) what was tried: every distinct layer shape under the other tile and other K splits (knobs c2w_tile / c2w_splitk), and the
      first layer (3 -> 64) on the existing conv2d_igemm_kernel (mvs_conv2d_fwd) against the Cin = 3 arm.
Each row: torch.cuda.Event pairs after warm-up, one pair per repetition; median, 10th / 90th percentile, spread.  The default of
SegDFF(hip_features=None) follows from (a) and (b): HIP only when its p90 is below the stock path's p10.
Writes one JSON object to profiles/vgg_features_timing.json and prints it.

--arith bf16: instead of (a)-(d), the opt-in arithmetic of the HIP trunk (csrc/conv2d_wide_bf16_kernels.h) beside the fp32 HIP
trunk MEASURED IN THE SAME RUN (before and after the mode; the yardstick is the better of the two), same protocol: whole call,
every layer (share of the 2.5 PFLOP/s bf16 MFMA peak), the forced arms of every distinct shape, and for SegDFF on seven seeded
textured images the relative L1 of the mode's heat maps against the "f32" route and the share of pixels whose arg-max label
agrees (recorded, not asserted).  A mode wins when its whole-call p90 is below the fp32 trunk's p10.  Writes
profiles/vgg_features_timing_arith.json (--out: another path)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

import mvs_amd  # noqa: F401
from mvs_amd import _lib, ops
from mvs_amd.jdacs.models.seg_dff import trunk_layers, vgg19_trunk

ap = argparse.ArgumentParser()
ap.add_argument("--arith", default="", help="comma-separated opt-in arithmetics to measure beside the fp32 HIP trunk: bf16")
ap.add_argument("--out", default="", help="where the JSON goes (default: profiles/vgg_features_timing[_arith].json)")
args = ap.parse_args()

REPS, WARMUP = 40, 8
PEAK = 157.3e12
PEAK_BF16 = 2.5e15
dev = torch.device("cuda:0")
lib = _lib.get()
torch.manual_seed(0)
net = vgg19_trunk().to(dev)
imgs = torch.rand(1, 7, 3, 512, 640, generator=torch.Generator().manual_seed(1)).to(dev)
b, nv = imgs.shape[:2]
layers = trunk_layers(net)
plan_layers = [(m.weight, m.bias, relu, pool) for m, relu, pool in layers]


def timed(fn, reps=REPS, warmup=WARMUP):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    q = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]
    return {"median_ms": q(0.5), "p10_ms": q(0.1), "p90_ms": q(0.9), "spread_ms": q(0.9) - q(0.1), "reps": reps}


def stock():
    with torch.no_grad():
        x = F.interpolate(imgs.reshape(b * nv, *imgs.shape[2:]), size=(224, 224), mode="bilinear", align_corners=False)
        f = net.features(x)
        c, h, w = f.shape[1:]
        return f.permute(0, 2, 3, 1).reshape(b, nv * h * w, c).float().contiguous()


def hip(arith="f32"):
    with torch.no_grad():
        x = ops.resize_bilinear_cl(imgs.reshape(b * nv, *imgs.shape[2:]), (224, 224))
        f = ops.conv_trunk_forward(ops.trunk_plan(plan_layers, x.shape, x, arith=arith), x)
        return f.view(b, -1, f.shape[3])


def layer_table(arith):
    """every layer of the HIP trunk on its own in one arithmetic + the other arms of every distinct shape -> (rows, tried)"""
    a = ops.wide_arith(arith)
    n, h, w, cin = 7, 224, 224, 3
    x = ops.resize_bilinear_cl(imgs.reshape(b * nv, *imgs.shape[2:]), (224, 224))
    rows, tried, seen = [], [], set()
    for m, relu, pool in layers:
        cout = m.out_channels
        packed = ops._wide_pack(lib, m.weight, x, a)
        y = torch.empty(n, h, w, cout, device=dev)

        def conv(x=x, packed=packed, y=y, cin=cin, cout=cout, h=h, w=w, m=m):
            ws = torch.empty(ops._wide_ws_floats(lib, n, h, w, cin, cout, a), device=dev)
            lib.call("mvs_conv2d_wide_fwd_arith", x.data_ptr(), packed.data_ptr(), m.bias.data_ptr(), y.data_ptr(), ws.data_ptr(), n, h, w, cin,
                     cout, 1, 0, a, ops._stream(x))

        lib.launch_trace()
        conv()
        arm = [t for t in lib.launch_trace() if "reduce" not in t][0]
        t = timed(conv)
        flop = 2.0 * n * h * w * cout * cin * 9
        on_bf = a != 0 and cin != 3
        rows.append(dict(layer="features.%d" % [k for k, mm in enumerate(net.features) if mm is m][0], shape="%dx%dx%d %d->%d" % (n, h, w, cin, cout),
                         arm=arm, gflop=flop / 1e9,
                         share_of_peak=flop / (PEAK_BF16 if on_bf else PEAK) / (t["median_ms"] * 1e-3),
                         peak="bf16 MFMA 2.5 PFLOP/s" if on_bf else "fp32 MFMA 157.3 TFLOP/s", **t))
        key = (h, w, cin, cout)
        if key not in seen and cin != 3:
            seen.add(key)
            variants = [dict(c2w_tile=1, c2w_splitk=1), dict(c2w_tile=2, c2w_splitk=1)]
            if h <= 28:
                variants += [dict(c2w_tile=1, c2w_splitk=s) for s in (2, 4, 8)]
            for kn in variants:
                with lib.tuning(**kn):
                    tv = timed(conv, reps=20, warmup=4)
                tried.append(dict(shape="%dx%dx%d %d->%d" % (n, h, w, cin, cout), knobs=kn, median_ms=tv["median_ms"], p10_ms=tv["p10_ms"],
                                  p90_ms=tv["p90_ms"]))
        x = y
        if pool:
            x, h, w = ops.maxpool2x2_cl(x), h // 2, w // 2
        cin = cout
    return rows, tried


def textured_images(seed=7):
    """seven 3x512x640 images of a few smooth blobs of different colour and stripe texture plus noise, in [0, 1]: what a k = 4
    clustering has something to separate on"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, 512), torch.linspace(0, 1, 640), indexing="ij")
    out = []
    for _ in range(7):
        img = torch.zeros(3, 512, 640)
        for _ in range(5):
            cx, cy, r = torch.rand(3, generator=g).tolist()
            fr, ph = 20 + 60 * float(torch.rand(1, generator=g)), 6.28 * float(torch.rand(1, generator=g))
            mask = (((xx - cx) ** 2 + (yy - cy) ** 2) < (0.15 + 0.25 * r) ** 2).float()
            col = torch.rand(3, 1, 1, generator=g)
            img = img * (1 - mask) + mask * col * (0.6 + 0.4 * torch.sin(fr * (xx * cx + yy * cy) + ph))
        out.append((img + 0.05 * torch.randn(3, 512, 640, generator=g)).clamp(0, 1))
    return torch.stack(out).unsqueeze(0)


def arith_report(modes):
    from mvs_amd.jdacs.models.seg_dff import SegDFF
    res = {"what": "HIP trunk of SegDFF in its opt-in arithmetic beside the fp32 HIP trunk of the same run: B=1 N=7, 3x512x640 images -> "
                   "224x224 -> VGG19 trunk -> [1,1372,512]; vgg19_trunk() weights of seed 0; whole call = resize + trunk",
           "device": torch.cuda.get_device_name(0), "bf16_mfma_peak_tflops": PEAK_BF16 / 1e12, "fp32_mfma_peak_tflops": PEAK / 1e12,
           "rule": "a mode wins when its whole-call p90 is below the fp32 trunk's p10 (the lower p10 of the two fp32 measurements)"}
    res["f32_before"] = timed(hip)
    for mode in modes:
        res[mode] = {"whole_call": timed(lambda: hip(mode))}
    res["f32_after"] = timed(hip)
    p10 = min(res["f32_before"]["p10_ms"], res["f32_after"]["p10_ms"])
    ref = hip()
    rows32, tried32 = layer_table("f32")
    res["f32_layers"], res["f32_d_tried"] = rows32, tried32
    heat32 = None
    timgs = textured_images().to(dev)
    with torch.no_grad():
        heat32 = SegDFF(4, net=net, hip_features=True)(timgs)
    for mode in modes:
        r = res[mode]
        r["p90_below_f32_p10"] = bool(r["whole_call"]["p90_ms"] < p10)
        out = hip(mode)
        r["relative_l1_features_vs_f32"] = float((out - ref).abs().sum() / ref.abs().sum())
        r["layers"], r["d_tried"] = layer_table(mode)
        r["sum_of_conv_layer_medians_ms"] = sum(x["median_ms"] for x in r["layers"])
        with torch.no_grad():
            heat = SegDFF(4, net=net, hip_features=True, feature_arith=mode)(timgs)
        r["segdff_heatmap_relative_l1_vs_f32"] = float((heat - heat32).abs().sum() / heat32.abs().sum())
        r["segdff_argmax_agreement"] = float((heat.argmax(-1) == heat32.argmax(-1)).float().mean())
    res["f32_sum_of_conv_layer_medians_ms"] = sum(x["median_ms"] for x in rows32)
    return res


if args.arith:
    res = arith_report([m for m in args.arith.split(",") if m])
    out = args.out or os.path.join(ROOT, "profiles", "vgg_features_timing_arith.json")
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    sys.exit(0)


res = {"what": "SegDFF feature extractor, B=1 N=7, 3x512x640 images -> 224x224 -> VGG19 trunk (16 convolutions, 4 pools) -> [1,1372,512]; "
               "vgg19_trunk() weights of seed 0", "device": torch.cuda.get_device_name(0), "fp32_mfma_peak_tflops": PEAK / 1e12}
torch.backends.cudnn.benchmark = False
res["a_stock_benchmark_off"] = timed(stock)
torch.backends.cudnn.benchmark = True
res["a_stock_benchmark_on"] = timed(stock)
torch.backends.cudnn.benchmark = False
pick = min(("a_stock_benchmark_off", "a_stock_benchmark_on"), key=lambda k: res[k]["median_ms"])
res["a_stock"] = dict(res[pick], picked=pick)
res["b_hip"] = timed(hip)
rel = float((hip() - stock()).abs().sum() / stock().abs().sum())
res["relative_l1_hip_vs_stock"] = rel
res["hip_p90_below_stock_p10"] = bool(res["b_hip"]["p90_ms"] < res["a_stock"]["p10_ms"])

# (c) per layer, (d) the other arms of every distinct shape
n, h, w, cin = 7, 224, 224, 3
x = ops.resize_bilinear_cl(imgs.reshape(b * nv, *imgs.shape[2:]), (224, 224))
rows, tried, seen = [], [], set()
total_gmac = 0.0
for i, (m, relu, pool) in enumerate(layers):
    cout = m.out_channels
    packed = ops._wide_pack(lib, m.weight, x)
    y = torch.empty(n, h, w, cout, device=dev)

    def conv(x=x, packed=packed, y=y, cin=cin, cout=cout, h=h, w=w, m=m):
        ws = torch.empty(ops._wide_ws_floats(lib, n, h, w, cin, cout), device=dev)
        lib.call("mvs_conv2d_wide_fwd", x.data_ptr(), packed.data_ptr(), m.bias.data_ptr(), y.data_ptr(), ws.data_ptr(), n, h, w, cin, cout, 1, 0,
                 ops._stream(x))

    lib.launch_trace()
    conv()
    arm = [t for t in lib.launch_trace() if "reduce" not in t][0]
    t = timed(conv)
    flop = 2.0 * n * h * w * cout * cin * 9
    total_gmac += flop / 2e9
    rows.append(dict(layer="features.%d" % [k for k, mm in enumerate(net.features) if mm is m][0], shape="%dx%dx%d %d->%d" % (n, h, w, cin, cout),
                     arm=arm, gflop=flop / 1e9, share_of_peak=flop / (t["median_ms"] * 1e-3) / PEAK, **t))
    key = (h, w, cin, cout)
    if key not in seen and cin != 3:
        seen.add(key)
        variants = [dict(c2w_tile=1, c2w_splitk=1), dict(c2w_tile=2, c2w_splitk=1)]
        if h <= 28:
            variants += [dict(c2w_tile=1, c2w_splitk=s) for s in (2, 4, 8)]
        for kn in variants:
            with lib.tuning(**kn):
                tv = timed(conv, reps=20, warmup=4)
            tried.append(dict(shape="%dx%dx%d %d->%d" % (n, h, w, cin, cout), knobs=kn, median_ms=tv["median_ms"], p10_ms=tv["p10_ms"],
                              p90_ms=tv["p90_ms"], share_of_peak=flop / (tv["median_ms"] * 1e-3) / PEAK))
    if cin == 3:
        xl = x.permute(0, 3, 1, 2)           # logical [N,3,H,W], channels-last in memory: the existing family's layout
        tv = timed(lambda: ops.conv2d_forward(xl, m.weight, m.bias), reps=20, warmup=4)
        tried.append(dict(shape="%dx%dx%d 3->64" % (n, h, w), knobs="conv2d_igemm_kernel (mvs_conv2d_fwd_wl, no ReLU)", median_ms=tv["median_ms"],
                          p10_ms=tv["p10_ms"], p90_ms=tv["p90_ms"], share_of_peak=flop / (tv["median_ms"] * 1e-3) / PEAK))
    x = y
    if pool:
        yp = torch.empty(n, h // 2, w // 2, cout, device=dev)
        tp = timed(lambda x=x, yp=yp, h=h, w=w, cout=cout: lib.call("mvs_maxpool2x2_cl", x.data_ptr(), yp.data_ptr(), n, h, w, cout, ops._stream(x)))
        rows.append(dict(layer="pool after it", shape="%dx%dx%d x%d" % (n, h, w, cout), arm="pool2x2",
                         gbytes_per_s=1.25 * n * h * w * cout * 4 / (tp["median_ms"] * 1e-3) / 1e9, **tp))
        x, h, w = yp, h // 2, w // 2
    cin = cout
res["work_gmac"] = total_gmac
res["c_layers"] = rows
res["c_sum_of_layer_medians_ms"] = sum(r["median_ms"] for r in rows)
res["c_pools_ms"] = sum(r["median_ms"] for r in rows if r["arm"] == "pool2x2")
res["b_share_of_peak"] = 2e9 * total_gmac / (res["b_hip"]["median_ms"] * 1e-3) / PEAK
res["d_tried"] = tried
out = args.out or os.path.join(ROOT, "profiles", "vgg_features_timing.json")
with open(out, "w") as fh:
    json.dump(res, fh, indent=1)
    fh.write("\n")
print(json.dumps(res))
