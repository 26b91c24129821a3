"""TEST INFRASTRUCTURE: the case table of the conv2d arms (csrc/conv2d.hip: c2_run_igemm, mvs_conv2d_dgrad_wl, mvs_conv2d_wgrad and
wg2_plan pick a template instantiation by channel counts, Cout tiles, the pixel-pair form, the BatchNorm epilogues and by knobs), at
the SMALLEST shapes at which these kernels can still go wrong -- tiles are 8 x 32 positions (4 x 32 for the batched weight
gradient's configs C / E / F), so 1x1, 1x2, 2x3, 7x31, 8x32, 9x33 (stride 2 also 2x1, 2x2, 3x3, 15x63, 16x64, 17x65).  Shared by

  * tests/test_gpu_conv2d_arms.py -- every case on the MI355X against an fp64 CPU reference (ATen's fp32 result is the yardstick), and
  * tests/test_conv2d_arm_dispatch.py -- the same calls on the emulation library: every trace with the kernel bodies skipped, the
    numbers for the cases of at most four tiles.

A case = one op at one shape; its `variants` are the knob settings / call forms under test, each with the EXACT launch trace it must
leave (written out here by hand from the layer's channel counts: `cc`, `nb` are stated per row, not computed by the dispatch's own
rule); `pairs` name variants compared on identical inputs: "equal" where the arithmetic order is provably the same (channels-last
against contiguous parameters, a weight image packed ahead of the call), "close" otherwise (2e-4 x scale, the conv3d file's bound)."""
import collections
import json
import os
import zlib

import torch
import torch.nn.functional as F

Variant = collections.namedtuple("Variant", "name knobs trace opts")
Case = collections.namedtuple("Case", "id op n hw cin cout ks stride opt variants pairs")

CL = torch.channels_last
TAIL = 1024                                   # canary elements behind every buffer the library writes
NAN_BITS = 0x7FC00000                         # torch's float("nan")
F64_BITS = 0x5A5A5A5A5A5A5A5A                 # the canary pattern of fp64 slot buffers
PACK = "conv2d_pack_weights_batch"
BATCH = ["conv2d_wgrad_batch", "conv2d_wgrad_batch_reduce"]
BATCH_XF = ["conv2d_wgrad_batch xf", "conv2d_wgrad_batch_reduce"]


def ig(ks, cc, nb, ep=""):
    return "conv2d_igemm k%d cc%d nb%d%s" % (ks, cc, nb, " " + ep if ep else "")


def pp(cc, ep=""):
    return "conv2d_igemm (pixel pairs) cc%d%s" % (cc, " " + ep if ep else "")


def wg(ks, cxp, nb):
    return "conv2d_wgrad k%d cxp%d nb%d" % (ks, cxp, nb)


def V(name, trace, knobs=None, **opts):
    return Variant(name, knobs or {}, list(trace), opts)


def _case(id, op, n, hw, cin, cout, ks, variants, pairs=(), **opt):
    return Case(id, op, n, hw, cin, cout, ks, 2 if ks == 5 else 1, opt, list(variants), list(pairs))


def _cl_pair(trace, knobs=None):
    """contiguous and channels-last parameters: the packed image is the same, so the outputs must be bit-identical"""
    return [V("contiguous", trace, knobs), V("channels_last", trace, knobs, wcl=True)], [("contiguous", "channels_last", "equal")]


# ---- forward, plain epilogue: every CC x NB of the 3x3 kernel, grid.y = 2 (Cout 64), two 32-channel chunks (Cin 64), scalar halo
# loads (Cin & 3), scalar stores (Cout & 3), a partly filled second Cout tile (Cout 20); the 5x5 stride-2 kernel ----
FWD = []
for _id, _n, _hw, _ci, _co, _cc, _nb in (
        ("3_16", 2, (7, 31), 3, 16, 4, 1), ("4_20", 1, (9, 33), 4, 20, 4, 2), ("5_16", 2, (2, 3), 5, 16, 8, 1), ("8_32", 2, (8, 32), 8, 32, 8, 2),
        ("13_6", 1, (9, 33), 13, 6, 16, 1), ("16_20", 2, (1, 2), 16, 20, 16, 2), ("20_3", 2, (7, 31), 20, 3, 32, 1),
        ("32_32", 1, (9, 33), 32, 32, 32, 2), ("64_64", 1, (8, 32), 64, 64, 32, 2), ("32_64", 2, (1, 1), 32, 64, 32, 2),
        ("64_1", 1, (9, 33), 64, 1, 32, 1), ("1_20", 2, (2, 3), 1, 20, 4, 2)):
    _vs, _ps = _cl_pair([ig(3, _cc, _nb)]) if _ci > 1 else ([V("default", [ig(3, _cc, _nb)])], [])
    FWD.append(_case("fwd_" + _id, "fwd", _n, _hw, _ci, _co, 3, _vs, _ps))
for _id, _n, _hw, _ci, _co, _nb in (("3_16", 2, (2, 1), 3, 16, 1), ("3_32", 1, (2, 2), 3, 32, 2), ("8_16", 2, (3, 3), 8, 16, 1),
                                    ("8_32", 1, (15, 63), 8, 32, 2), ("16_16", 1, (16, 64), 16, 16, 1), ("16_32", 1, (17, 65), 16, 32, 2),
                                    ("8_16_tile", 2, (9, 33), 8, 16, 1)):
    _vs, _ps = _cl_pair([ig(5, 8, _nb)])
    FWD.append(_case("fwd5_" + _id, "fwd", _n, _hw, _ci, _co, 5, _vs, _ps))
# bias, and LeakyReLU 0.1 behind it (mvs_conv2d_lrelu_fwd), inputs on both sides of zero, Cout 1 / 16 / 64
for _id, _n, _hw, _ci, _co, _lab in (("8_1", 2, (7, 31), 8, 1, pp(8)), ("16_16", 1, (9, 33), 16, 16, ig(3, 16, 1)), ("32_64", 2, (2, 3), 32, 64, ig(3, 32, 2))):
    FWD.append(_case("fwd_bias_" + _id, "fwd", _n, _hw, _ci, _co, 3, [V("default", [_lab])], bias=True))
    FWD.append(_case("fwd_lrelu_" + _id, "fwd", _n, _hw, _ci, _co, 3, [V("default", [_lab])], bias=True, slope=0.1))

# ---- pixel pairs (Cout <= 8 and Cin <= 8; knob conv2d_pp 1 against 0 on identical inputs): W = 1 / 31 / 33 puts the pair across the
# right edge; forward and stride-1 input gradient (the transposed, flipped image) ----
PIXEL_PAIRS = []
for _op, _id, _n, _hw, _ci, _co, _cc in (
        ("fwd", "1_1", 2, (1, 1), 1, 1, 4), ("fwd", "3_8", 2, (7, 31), 3, 8, 4), ("fwd", "4_3", 1, (2, 1), 4, 3, 4), ("fwd", "8_8", 1, (9, 33), 8, 8, 8),
        ("fwd", "5_6", 2, (8, 31), 5, 6, 8), ("dgrad", "8_8", 1, (9, 33), 8, 8, 8), ("dgrad", "8_3", 2, (7, 31), 8, 3, 4), ("dgrad", "3_5", 2, (1, 1), 3, 5, 8)):
    # (an input gradient is a forward pass on gy: its GEMM has the layer's Cout as input channels -- cc -- and the layer's Cin as columns)
    _vs = [V("pixel_pairs", [pp(_cc)], {"conv2d_pp": 1}), V("plain", [ig(3, _cc, 1)], {"conv2d_pp": 0})]
    _ps = [("pixel_pairs", "plain", "close")]
    if _id == "8_8":
        _vs.append(V("pixel_pairs_channels_last", [pp(_cc)], {"conv2d_pp": 1}, wcl=True))
        _ps.append(("pixel_pairs", "pixel_pairs_channels_last", "equal"))
    PIXEL_PAIRS.append(_case("pp_%s_%s" % (_op, _id), _op, _n, _hw, _ci, _co, 3, _vs, _ps))

# ---- stride-1 input gradient, plain kernel: layer Cin -> Cout, GEMM cc from the layer's Cout, nb from its Cin ----
DGRAD = []
for _id, _n, _hw, _ci, _co, _cc, _nb in (
        ("16_3", 2, (7, 31), 16, 3, 4, 1), ("20_4", 1, (9, 33), 20, 4, 4, 2), ("16_5", 2, (2, 3), 16, 5, 8, 1), ("32_8", 2, (8, 32), 32, 8, 8, 2),
        ("6_13", 1, (9, 33), 6, 13, 16, 1), ("20_16", 2, (1, 2), 20, 16, 16, 2), ("3_20", 2, (7, 31), 3, 20, 32, 1),
        ("32_32", 1, (9, 33), 32, 32, 32, 2), ("64_64", 1, (8, 32), 64, 64, 32, 2), ("1_64", 1, (9, 33), 1, 64, 32, 1)):
    _vs, _ps = _cl_pair([ig(3, _cc, _nb)]) if _co > 1 and _ci > 1 else ([V("default", [ig(3, _cc, _nb)])], [])
    DGRAD.append(_case("dgrad_" + _id, "dgrad", _n, _hw, _ci, _co, 3, _vs, _ps))

# ---- STATS (mvs_conv2d_fwd_stats; `packed`: the weight image written ahead by mvs_conv2d_pack_weights_batch): groups 1, N, and
# N = 4 in 2 groups; `nslots` of the caller-owned call: fewer slot rows than workgroups (the blockIdx.x & (nslots - 1) wrap) and more ----
STATS = []
for _id, _n, _hw, _ci, _co, _ks, _lab, _g, _ns in (
        ("3_8", 2, (7, 31), 3, 8, 3, pp(4, "stats"), 2, 2), ("8_8", 4, (9, 33), 8, 8, 3, pp(8, "stats"), 2, 2),
        ("3_16", 2, (9, 33), 3, 16, 3, ig(3, 4, 1, "stats"), 1, 16), ("4_32", 2, (2, 3), 4, 32, 3, ig(3, 4, 2, "stats"), 2, 1),
        ("8_16", 4, (8, 32), 8, 16, 3, ig(3, 8, 1, "stats"), 2, 4), ("5_32", 1, (9, 33), 5, 32, 3, ig(3, 8, 2, "stats"), 1, 2),
        ("16_16", 2, (1, 1), 16, 16, 3, ig(3, 16, 1, "stats"), 2, 8), ("13_32", 2, (7, 31), 13, 32, 3, ig(3, 16, 2, "stats"), 1, 1),
        ("32_16", 1, (1, 2), 32, 16, 3, ig(3, 32, 1, "stats"), 1, 2), ("32_64", 2, (9, 33), 32, 64, 3, ig(3, 32, 2, "stats"), 2, 4),
        ("8_16_k5", 2, (17, 65), 8, 16, 5, ig(5, 8, 1, "stats"), 2, 2), ("16_32_k5", 4, (15, 63), 16, 32, 5, ig(5, 8, 2, "stats"), 2, 16),
        ("3_8_k5", 1, (3, 3), 3, 8, 5, ig(5, 8, 1, "stats"), 1, 4)):
    STATS.append(_case("stats_" + _id, "stats", _n, _hw, _ci, _co, _ks,
                       [V("in_call", [_lab]), V("packed", [PACK, _lab], packed=True), V("packed_channels_last", [PACK, _lab], packed=True, wcl=True)],
                       [("in_call", "packed", "equal"), ("in_call", "packed_channels_last", "equal")], groups=_g, nslots=_ns))

# ---- XF (mvs_conv2d_fwd_stats_xf): x is the raw output of the BatchNorm + ReLU block in front; negative scales on some channels,
# strictly positive shifts on others (a transformed zero padding, or a clip with the wrong sign, is then visibly off) ----
XF = []
for _id, _n, _hw, _ci, _co, _ks, _lab, _g in (
        ("8_8", 2, (9, 33), 8, 8, 3, pp(8, "stats+xf"), 2), ("8_16_k5", 2, (17, 65), 8, 16, 5, ig(5, 8, 1, "stats+xf"), 1),
        ("16_16", 2, (7, 31), 16, 16, 3, ig(3, 16, 1, "stats+xf"), 2), ("32_32", 4, (8, 32), 32, 32, 3, ig(3, 32, 2, "stats+xf"), 2),
        ("4_16", 1, (2, 3), 4, 16, 3, ig(3, 4, 1, "stats+xf"), 1), ("4_32", 2, (1, 1), 4, 32, 3, ig(3, 4, 2, "stats+xf"), 2),
        ("8_16", 1, (9, 33), 8, 16, 3, ig(3, 8, 1, "stats+xf"), 1), ("8_32", 2, (1, 2), 8, 32, 3, ig(3, 8, 2, "stats+xf"), 1),
        ("16_32", 2, (9, 33), 16, 32, 3, ig(3, 16, 2, "stats+xf"), 2), ("32_16", 1, (7, 31), 32, 16, 3, ig(3, 32, 1, "stats+xf"), 1),
        ("16_32_k5", 2, (2, 2), 16, 32, 5, ig(5, 8, 2, "stats+xf"), 2)):
    XF.append(_case("xf_" + _id, "xf", _n, _hw, _ci, _co, _ks, [V("in_call", [_lab]), V("packed", [PACK, _lab], packed=True)],
                    [("in_call", "packed", "equal")], groups=_g, nslots=4))

# ---- BST (mvs_conv2d_dgrad_bnstats): layer Cin -> Cout; 6 -> 16 takes the scalar bn_raw loads ----
BST = []
for _id, _n, _hw, _ci, _co, _lab, _g in (
        ("8_8", 2, (9, 33), 8, 8, pp(8, "stats+bst"), 2), ("8_4", 2, (7, 31), 8, 4, pp(4, "stats+bst"), 1),
        ("16_16", 2, (8, 32), 16, 16, ig(3, 16, 1, "stats+bst"), 2), ("32_32", 1, (9, 33), 32, 32, ig(3, 32, 2, "stats+bst"), 1),
        ("6_16", 2, (7, 31), 6, 16, ig(3, 16, 1, "stats+bst"), 2), ("16_4", 1, (2, 3), 16, 4, ig(3, 4, 1, "stats+bst"), 1),
        ("32_4", 2, (1, 1), 32, 4, ig(3, 4, 2, "stats+bst"), 2), ("16_8", 2, (1, 2), 16, 8, ig(3, 8, 1, "stats+bst"), 1),
        ("20_8", 1, (9, 33), 20, 8, ig(3, 8, 2, "stats+bst"), 1), ("32_16", 2, (2, 3), 32, 16, ig(3, 16, 2, "stats+bst"), 2),
        ("16_32", 2, (9, 33), 16, 32, ig(3, 32, 1, "stats+bst"), 1)):
    BST.append(_case("bst_" + _id, "bst", _n, _hw, _ci, _co, 3, [V("default", [_lab])], groups=_g, nslots=2))

# ---- stride-2 input gradient of the 5x5 layers, all three forms (knob conv2d_s2_mfma 2 / 1 / 0); layer Cin -> Cout, cc from the
# layer's Cout (<= 4 falls through the `else`), nb from its Cin.  The odd parity classes have one row / column fewer, or none ----
DGRAD_S2 = []
for _id, _n, _hw, _ci, _co, _cc, _nb in (
        ("8_3", 2, (3, 3), 8, 3, 4, 1), ("20_4", 1, (15, 63), 20, 4, 4, 2), ("3_5", 2, (2, 1), 3, 5, 8, 1), ("32_8", 1, (16, 64), 32, 8, 8, 2),
        ("16_16", 1, (17, 65), 16, 16, 16, 1), ("20_16", 2, (2, 2), 20, 16, 16, 2), ("8_32", 1, (15, 63), 8, 32, 32, 1),
        ("32_32", 1, (17, 65), 32, 32, 32, 2), ("16_8_1x1", 2, (1, 1), 16, 8, 8, 1), ("8_8_1x2", 2, (1, 2), 8, 8, 8, 1),
        ("3_16_9x33", 2, (9, 33), 3, 16, 16, 1), ("8_16_7x31", 1, (7, 31), 8, 16, 16, 1)):
    _lab = " cc%d nb%d" % (_cc, _nb)
    DGRAD_S2.append(_case("dgrad_s2_" + _id, "dgrad", _n, _hw, _ci, _co, 5,
                          [V("one_pass", ["conv2d_dgrad_s2_one_pass" + _lab], {"conv2d_s2_mfma": 2}),
                           V("one_pass_channels_last", ["conv2d_dgrad_s2_one_pass" + _lab], {"conv2d_s2_mfma": 2}, wcl=True),
                           V("classes", ["conv2d_dgrad_s2_classes" + _lab], {"conv2d_s2_mfma": 1}),
                           V("classes_channels_last", ["conv2d_dgrad_s2_classes" + _lab], {"conv2d_s2_mfma": 1}, wcl=True),
                           V("direct", ["conv2d_dgrad_s2"], {"conv2d_s2_mfma": 0})],
                          [("one_pass", "one_pass_channels_last", "equal"), ("classes", "classes_channels_last", "equal"),
                           ("one_pass", "classes", "close"), ("one_pass", "direct", "close")]))

# ---- per-layer weight gradient: all twelve instantiations, CX / CG not multiples of 4 (5 -> 6, 13 -> 3), the 64-channel slices
# (x0 / g0 non-zero), a workgroup that walks >= 3 ragged tiles (knob wgrad2d_groups 1 / 3 over 8 tiles) ----
NARROW, WIDE = "conv2d_wgrad_reduce narrow", "conv2d_wgrad_reduce wide"
WGRAD = []
for _id, _n, _hw, _ci, _co, _ks, _cxp, _nb in (
        ("3_8", 2, (7, 31), 3, 8, 3, 4, 1), ("4_20", 1, (9, 33), 4, 20, 3, 4, 2), ("5_6", 2, (2, 3), 5, 6, 3, 8, 1), ("8_32", 2, (8, 32), 8, 32, 3, 8, 2),
        ("13_3", 1, (9, 33), 13, 3, 3, 16, 1), ("16_20", 2, (1, 2), 16, 20, 3, 16, 2), ("32_16", 2, (1, 1), 32, 16, 3, 32, 1),
        ("29_32", 1, (9, 33), 29, 32, 3, 32, 2), ("8_16_k5", 1, (15, 63), 8, 16, 5, 8, 1), ("5_32_k5", 2, (3, 3), 5, 32, 5, 8, 2),
        ("16_8_k5", 1, (16, 64), 16, 8, 5, 16, 1), ("13_30_k5", 1, (17, 65), 13, 30, 5, 16, 2), ("8_16_k5_2x1", 2, (2, 1), 8, 16, 5, 8, 1)):
    WGRAD.append(_case("wgrad_" + _id, "wgrad", _n, _hw, _ci, _co, _ks, [V("default", [wg(_ks, _cxp, _nb), NARROW])]))
WGRAD += [
    _case("wgrad_64_64", "wgrad", 1, (9, 33), 64, 64, 3, [V("default", [wg(3, 32, 2)] * 4 + [NARROW])]),
    _case("wgrad_64_16", "wgrad", 2, (7, 31), 64, 16, 3, [V("default", [wg(3, 32, 1)] * 2 + [NARROW])]),
    _case("wgrad_16_64", "wgrad", 2, (2, 3), 16, 64, 3, [V("default", [wg(3, 16, 2)] * 2 + [NARROW])]),
    _case("wgrad_groups_16_16", "wgrad", 2, (9, 33), 16, 16, 3,
          [V("one_tile_each", [wg(3, 16, 1), NARROW]), V("groups_3", [wg(3, 16, 1), NARROW], {"wgrad2d_groups": 3}),
           V("groups_1", [wg(3, 16, 1), NARROW], {"wgrad2d_groups": 1})],
          [("one_tile_each", "groups_3", "close"), ("one_tile_each", "groups_1", "close")]),
    _case("wgrad_groups_8_16_k5", "wgrad", 2, (17, 65), 8, 16, 5,
          [V("one_tile_each", [wg(5, 8, 1), NARROW]), V("groups_3", [wg(5, 8, 1), NARROW], {"wgrad2d_groups": 3})],
          [("one_tile_each", "groups_3", "close")]),
]
# the reduce switch (groups > 16): 1 x 24 x 192 = 18 tiles; knob 16 -> 16 partial images (narrow), 17 and the default (18) -> wide.
# 1 x 40 x 416 = 65 tiles: 49 and 65 partial images sit on the `p + 48 < nparts` boundary of the wide reduce's unrolled loop
WGRAD_REDUCE = [
    _case("wgrad_reduce_18_tiles", "wgrad", 1, (24, 192), 8, 16, 3,
          [V("narrow_16", [wg(3, 8, 1), NARROW], {"wgrad2d_groups": 16}), V("wide_17", [wg(3, 8, 1), WIDE], {"wgrad2d_groups": 17}),
           V("wide_18", [wg(3, 8, 1), WIDE])],
          [("narrow_16", "wide_17", "close"), ("narrow_16", "wide_18", "close")]),
    _case("wgrad_reduce_65_tiles", "wgrad", 1, (40, 416), 3, 8, 3,
          [V("wide_49", [wg(3, 4, 1), WIDE], {"wgrad2d_groups": 49}), V("wide_65", [wg(3, 4, 1), WIDE]),
           V("wide_48", [wg(3, 4, 1), WIDE], {"wgrad2d_groups": 48})],
          [("wide_65", "wide_49", "close"), ("wide_65", "wide_48", "close")]),
]

# ---- batched weight gradient (wg2_plan): layers = (Cin, Cout, ks, H x W, parameter channels-last, x is raw + statistics) ----
_ONE = [V("default", BATCH)]
_FEATURENET = [(3, 8, 3, (20, 40), False, False), (8, 8, 3, (20, 40), True, False), (8, 16, 5, (20, 40), False, False),
               (16, 16, 3, (10, 20), True, False), (16, 16, 3, (10, 20), False, False), (16, 32, 5, (10, 20), True, False),
               (32, 32, 3, (5, 10), False, False), (32, 32, 3, (5, 10), True, False)]
WGRAD_BATCH = [
    # each of the six configs alone (one launch class is then empty), CG 4 / 8 / 12 / 16 for the NB = 1 configs, 20 / 32 for NB = 2
    _case("batch_A_3_4", "wgrad_batch", 1, None, 0, 0, 3, _ONE, layers=[(3, 4, 3, (7, 31), False, False)]),
    _case("batch_B_8_8", "wgrad_batch", 1, None, 0, 0, 3, _ONE, layers=[(8, 8, 3, (9, 33), True, False)]),
    _case("batch_C_8_12", "wgrad_batch", 1, None, 0, 0, 3, _ONE, layers=[(8, 12, 5, (17, 65), False, False)]),
    _case("batch_D_16_16", "wgrad_batch", 1, None, 0, 0, 3, _ONE, layers=[(16, 16, 3, (2, 3), True, False)]),
    _case("batch_E_16_20", "wgrad_batch", 1, None, 0, 0, 3, _ONE, layers=[(16, 20, 5, (15, 63), False, False)]),
    _case("batch_F_32_32", "wgrad_batch", 1, None, 0, 0, 3, _ONE, layers=[(32, 32, 3, (9, 33), True, False)]),
    _case("batch_F_32_20", "wgrad_batch", 2, None, 0, 0, 3, _ONE, layers=[(32, 20, 3, (1, 1), False, False)]),
    _case("batch_C_8_16_1x2", "wgrad_batch", 2, None, 0, 0, 3, _ONE, layers=[(8, 16, 5, (1, 2), True, False)]),
    # FeatureNet's eight layers at N = 2, 20 x 40 (levels 20 x 40, 10 x 20, 5 x 10); knob wgrad2d_batch 1 (clamped to the layer
    # count: one workgroup per layer walks all its tiles), 6 (tpw > 1, ragged last workgroup), default (one tile per workgroup)
    # `ws_floats`: the workspace the plan must ask for = sum over the layers of workgroups x ROWSP x CGP, worked out by hand from
    # tiles per workgroup = ceil(tiles / share), share = budget x the layer's part of the cost (tiles x (NPOS / 4 x MTT x NB + 96)):
    #   default: one tile per workgroup, 12 12 6 4 4 4 4 4 workgroups; budgets 1 and 6 are both below the 8 layers -> 8: 1 1 1 1 1 2 1 1
    #   (conv5, the costliest, gets two); 20: 2 3 2 2 2 4 2 2 workgroups of 6 4 3 2 2 1 2 2 tiles (a floor would make it 2 3 2 2 2 4 4 4)
    _case("batch_featurenet", "wgrad_batch", 2, None, 0, 0, 3,
          [V("default", BATCH, ws_floats=184832), V("budget_1", BATCH, {"wgrad2d_batch": 1}, ws_floats=53760),
           V("budget_6", BATCH, {"wgrad2d_batch": 6}, ws_floats=53760), V("budget_20", BATCH, {"wgrad2d_batch": 20}, ws_floats=108800)],
          [("default", "budget_1", "close"), ("default", "budget_6", "close"), ("default", "budget_20", "close")], layers=_FEATURENET),
    # a ragged last workgroup: 8 tiles of the 8 -> 8 layer over 3 workgroups (3 + 3 + 2), the 16 -> 16 layer's 2 tiles in one:
    # 3 x 80 x 16 + 1 x 144 x 16 floats (a floor would give the first layer 4 workgroups of 2)
    _case("batch_ragged_split", "wgrad_batch", 2, None, 0, 0, 3,
          [V("default", BATCH, ws_floats=8 * 80 * 16 + 2 * 144 * 16), V("budget_4", BATCH, {"wgrad2d_batch": 4}, ws_floats=3 * 80 * 16 + 144 * 16)],
          [("default", "budget_4", "close")], layers=[(8, 8, 3, (9, 33), False, False), (16, 16, 3, (7, 31), True, False)]),
    # _xf: raw input + statistics on some layers, None on others; 1 and 2 statistics groups
    _case("batch_xf_g1", "wgrad_batch", 2, None, 0, 0, 3, [V("default", BATCH_XF), V("budget_3", BATCH_XF, {"wgrad2d_batch": 3})],
          [("default", "budget_3", "close")], groups=1,
          layers=[(8, 8, 3, (9, 33), False, True), (16, 16, 3, (7, 31), True, False), (32, 32, 3, (9, 33), False, True), (8, 16, 5, (17, 65), True, True)]),
    _case("batch_xf_g2", "wgrad_batch", 4, None, 0, 0, 3, [V("default", BATCH_XF)], groups=2,
          layers=[(3, 8, 3, (7, 31), False, False), (16, 16, 3, (8, 32), False, True), (16, 32, 5, (15, 63), True, True), (32, 20, 3, (2, 3), False, True)]),
]

GROUPS = collections.OrderedDict([("FWD", FWD), ("PIXEL_PAIRS", PIXEL_PAIRS), ("DGRAD", DGRAD), ("STATS", STATS), ("XF", XF), ("BST", BST),
                                  ("DGRAD_S2", DGRAD_S2), ("WGRAD", WGRAD), ("WGRAD_REDUCE", WGRAD_REDUCE), ("WGRAD_BATCH", WGRAD_BATCH)])
ALL = [c for grp in GROUPS.values() for c in grp]

# every launch label of csrc/conv2d.hip's narrow family (C2_IGEMM_LABEL, C2_K5_LABEL, C2_PP_LABEL, C2_S2D_LABEL, C2_S2C_LABEL,
# C2_WGRAD_LABEL and the literals of mvs_conv2d_wgrad / wg2_run / mvs_conv2d_pack_weights_batch / the direct stride-2 form)
ARM_LABELS = tuple(
    [ig(3, cc, nb, ep) for cc in (4, 8, 16, 32) for nb in (1, 2) for ep in ("", "stats", "stats+xf", "stats+bst")]
    + [ig(5, 8, nb, ep) for nb in (1, 2) for ep in ("", "stats", "stats+xf")]
    + [pp(4), pp(4, "stats"), pp(4, "stats+bst"), pp(8), pp(8, "stats"), pp(8, "stats+xf"), pp(8, "stats+bst")]
    + ["conv2d_dgrad_s2_%s cc%d nb%d" % (f, cc, nb) for f in ("one_pass", "classes") for cc in (4, 8, 16, 32) for nb in (1, 2)]
    + ["conv2d_dgrad_s2"]
    + [wg(3, cxp, nb) for cxp in (4, 8, 16, 32) for nb in (1, 2)] + [wg(5, cxp, nb) for cxp in (8, 16) for nb in (1, 2)]
    + [NARROW, WIDE, "conv2d_wgrad_batch", "conv2d_wgrad_batch xf", "conv2d_wgrad_batch_reduce", PACK])


# what mvs_conv2d_wgrad has no instantiation for (ks, Cin): the 3x3 slices that round to 12 / 20 / 24 / 28 channels, the 5x5 slices
# that round to anything but 8 / 16 -- and a sample of what it serves
WGRAD_GAP = [(3, 9), (3, 12), (3, 17), (3, 20), (3, 24), (3, 28), (5, 1), (5, 3), (5, 4), (5, 9), (5, 12), (5, 17), (5, 32), (5, 64)]
WGRAD_SERVED = [(3, c) for c in (1, 3, 4, 5, 8, 13, 16, 29, 32, 64)] + [(5, c) for c in (5, 8, 13, 16)]


def ids(cases):
    return [c.id for c in cases]


def out_hw(hw, stride):
    return tuple(hw) if stride == 1 else ((hw[0] - 1) // 2 + 1, (hw[1] - 1) // 2 + 1)


def tiles(case):
    """workgroup tiles of the case's largest launch (the emulation runs a thread per lane: its numeric test takes <= 4)"""
    def one(n, hw, stride, th):
        ho, wo = out_hw(hw, stride)
        return n * ((ho + th - 1) // th) * ((wo + 31) // 32)
    if case.op == "wgrad_batch":
        return sum(one(case.n, hw, 2 if ks == 5 else 1, 4 if (ks == 5 or cin == 32) else 8) for cin, _, ks, hw, _, _ in case.opt["layers"])
    if case.op in ("dgrad", "bst") and case.stride == 2:
        return one(case.n, ((case.hw[0] + 1) // 2, (case.hw[1] + 1) // 2), 1, 8) * 4
    if case.op in ("dgrad", "bst"):
        return one(case.n, case.hw, 1, 8) * (2 if case.cin == 64 else 1)
    if case.op == "wgrad":
        return one(case.n, case.hw, case.stride, 8) * (case.cin // 32 or 1) * (case.cout // 32 or 1)
    return one(case.n, case.hw, case.stride, 8) * (2 if case.cout == 64 else 1)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def _in_stats(g, groups, c):
    """[groups, 4, c] (mean, invstd, scale, shift) of a BatchNorm block: negative scales on odd channels, a strictly positive shift on
    every third channel, another set per group"""
    mean, invstd = torch.randn(groups, c, generator=g) * 0.2, 0.5 + torch.rand(groups, c, generator=g)
    scale = (0.5 + torch.rand(groups, c, generator=g)) * torch.where(torch.arange(c) % 2 == 1, -1.0, 1.0)
    shift = torch.randn(groups, c, generator=g) * 0.3
    shift[:, ::3] = shift[:, ::3].abs() + 0.25
    return torch.stack([mean, invstd, scale, shift], 1).contiguous()


def make_inputs(case):
    """fp32 CPU tensors of the case, seeded by its id; activations channels-last like the product's"""
    g = torch.Generator().manual_seed(zlib.crc32(case.id.encode()))
    rn = lambda *s: torch.randn(*s, generator=g)
    groups = case.opt.get("groups", 1)
    if case.op == "wgrad_batch":
        inp = {"xs": [], "gys": [], "ws": [], "x_stats": []}
        for cin, cout, ks, hw, wcl, xf in case.opt["layers"]:
            ho, wo = out_hw(hw, 2 if ks == 5 else 1)
            inp["xs"].append(rn(case.n, cin, *hw).contiguous(memory_format=CL))
            inp["gys"].append(rn(case.n, cout, ho, wo).contiguous(memory_format=CL))
            inp["ws"].append(torch.zeros(cout, cin, ks, ks))
            inp["x_stats"].append(_in_stats(g, groups, cin) if xf else None)
        return inp
    ho, wo = out_hw(case.hw, case.stride)
    inp = {"w": rn(case.cout, case.cin, case.ks, case.ks) * 0.2}
    if case.op in ("fwd", "stats", "xf", "wgrad"):
        inp["x"] = rn(case.n, case.cin, *case.hw).contiguous(memory_format=CL)
    if case.op in ("dgrad", "bst", "wgrad"):
        inp["gy"] = rn(case.n, case.cout, ho, wo).contiguous(memory_format=CL)
    if case.opt.get("bias"):
        inp["bias"] = rn(case.cout) * 0.3
    if case.op == "xf":
        inp["in_stats"] = _in_stats(g, groups, case.cin)
    if case.op == "bst":
        raw = rn(case.n, case.cin, *case.hw).contiguous(memory_format=CL)
        gamma, beta = 0.5 + torch.rand(case.cin, generator=g), rn(case.cin) * 0.3
        rg = raw.view(groups, case.n // groups, case.cin, *case.hw)
        mean, var = rg.mean(dim=(1, 3, 4)), rg.var(dim=(1, 3, 4), unbiased=False)
        invstd = torch.rsqrt(var + 1e-5)
        inp["raw"] = raw
        inp["stats"] = torch.stack([mean, invstd, gamma * invstd, beta - mean * gamma * invstd], 1).contiguous()     # [G, 4, Cin]
    return inp


def to_device(inp, dev):
    mv = lambda v: v.to(dev) if torch.is_tensor(v) else ([mv(t) for t in v] if isinstance(v, list) else v)
    out = {k: mv(v) for k, v in inp.items()}
    for k in ("x", "gy", "raw"):                    # (.to keeps the strides; a one-channel or one-pixel image is its own channels-last form)
        if k in out:
            out[k] = out[k].contiguous(memory_format=CL)
    return out


# ---- reference: plain torch on the CPU in `dtype` (float64 = the truth, float32 = the yardstick) ---------------------------------
def _per_image(stats, row, n, dtype):
    groups = stats.shape[0]
    return stats[torch.arange(n) // (n // groups), row].to(dtype)[:, :, None, None]


def _normalised(x, stats, dtype):
    """relu(x * scale + shift) with the statistics of each image's group"""
    n = x.shape[0]
    return torch.relu(x.to(dtype) * _per_image(stats, 2, n, dtype) + _per_image(stats, 3, n, dtype))


def _wgrad_ref(x, gy, wshape, stride, dtype):
    w = torch.zeros(wshape, dtype=dtype, requires_grad=True)
    F.conv2d(x, w, stride=stride, padding=wshape[2] // 2).backward(gy.to(dtype))
    return w.grad


def reference(case, inp, dtype):
    """-> {"out": tensor (list of tensors for wgrad_batch), "stats": [G, 2, C] backward sums of a BST case, else None}"""
    c = lambda t: t.to(dtype).contiguous()
    pad = case.ks // 2
    if case.op == "wgrad_batch":
        outs = []
        for (cin, cout, ks, hw, wcl, xf), x, gy, st in zip(case.opt["layers"], inp["xs"], inp["gys"], inp["x_stats"]):
            xin = _normalised(x, st, dtype) if st is not None else c(x)
            outs.append(_wgrad_ref(xin.contiguous(), c(gy), (cout, cin, ks, ks), 2 if ks == 5 else 1, dtype))
        return {"out": outs, "stats": None}
    w = c(inp["w"])
    if case.op in ("fwd", "stats", "xf"):
        x = _normalised(inp["x"], inp["in_stats"], dtype).contiguous() if case.op == "xf" else c(inp["x"])
        y = F.conv2d(x, w, c(inp["bias"]) if "bias" in inp else None, stride=case.stride, padding=pad)
        if case.opt.get("slope") is not None:
            y = F.leaky_relu(y, case.opt["slope"])
        return {"out": y, "stats": None}
    if case.op == "wgrad":
        return {"out": _wgrad_ref(c(inp["x"]), inp["gy"], tuple(w.shape), case.stride, dtype), "stats": None}
    x0 = torch.zeros(case.n, case.cin, *case.hw, dtype=dtype, requires_grad=True)
    (gx,) = torch.autograd.grad(F.conv2d(x0, w, stride=case.stride, padding=pad), x0, c(inp["gy"]))
    if case.op == "dgrad":
        return {"out": gx, "stats": None}
    # BST: gx is the complete gradient w.r.t. relu(bn(raw)); the slots get sum(dyh) and sum(dyh * xhat) per group, dyh = gx where the
    # block's output was positive.  The ReLU mask exactly as the kernel forms it (fp32 multiply, then add, no contraction)
    raw, st, n = inp["raw"], inp["stats"], case.n
    active = raw * _per_image(st, 2, n, torch.float32) + _per_image(st, 3, n, torch.float32) > 0
    dyh = gx * active
    xhat = (raw.to(dtype) - _per_image(st, 0, n, dtype)) * _per_image(st, 1, n, dtype)
    groups = st.shape[0]
    grp = lambda t: t.reshape(groups, n // groups, case.cin, *case.hw).sum(dim=(1, 3, 4))
    return {"out": gx, "stats": torch.stack([grp(dyh), grp(dyh * xhat)], 1)}


# ---- the op through mvs_amd.ops ---------------------------------------------------------------------------------------------
def _weight(w, v):
    return w.contiguous(memory_format=CL) if v.opts.get("wcl") else w.contiguous()


def run(case, inp, lib, v):
    """variant `v` of the case through the product's wrappers (knobs are the caller's business: `with lib.tuning(**v.knobs)`), on the
    device the tensors of `inp` live on -> {"out", "slots"}"""
    from mvs_amd import ops
    groups = case.opt.get("groups", 1)
    if case.op == "wgrad_batch":
        ws = [w.contiguous(memory_format=CL) if lay[4] else w for w, lay in zip(inp["ws"], case.opt["layers"])]
        strides = [2 if lay[2] == 5 else 1 for lay in case.opt["layers"]]
        gws = ops.conv2d_wgrad_batch(inp["xs"], inp["gys"], ws, strides, x_stats=inp["x_stats"], groups=groups)
        for gw, w in zip(gws, ws):
            assert gw.stride() == w.stride(), "the gradient takes the parameter's strides"
        return {"out": gws, "slots": None}
    w = _weight(inp["w"], v)
    if case.op == "fwd":
        return {"out": ops.conv2d_forward(inp["x"], w, inp.get("bias"), case.stride, negative_slope=case.opt.get("slope")), "slots": None}
    if case.op in ("stats", "xf"):
        packed = ops.pack_conv2d_weights([w], [case.stride], inp["x"])[0] if v.opts.get("packed") else None
        y, slots = ops.conv2d_forward(inp["x"], w, None, case.stride, want_stats=True, groups=groups, packed_ws=packed, in_stats=inp.get("in_stats"))
        return {"out": y, "slots": slots}
    if case.op == "wgrad":
        return {"out": ops.conv2d_wgrad(inp["x"], inp["gy"], tuple(w.shape), case.stride), "slots": None}
    in_shape = (case.n, case.cin) + tuple(case.hw)
    if case.op == "dgrad":
        return {"out": ops.conv2d_dgrad(inp["gy"], w, in_shape, case.stride), "slots": None}
    slots = torch.zeros((groups, case.opt["nslots"], 2, case.cin), dtype=torch.float64, device=inp["gy"].device)
    gx = ops.conv2d_dgrad(inp["gy"], w, in_shape, 1, bn=(inp["raw"], inp["stats"], slots), groups=groups)
    return {"out": gx, "slots": slots}


# ---- the op through lib.call on buffers the test owns: canaries ---------------------------------------------------------------
class Canaries:
    """Buffers with a tail of TAIL extra elements behind the size the library was promised: floats are NaN throughout (an output
    element the kernel skipped, or a workspace element it read without writing, shows), fp64 slots are zero with a fixed bit pattern
    in the tail.  check(): every tail unchanged -- a workspace query that is too small, or a dead lane of a ragged tile that stores,
    lands there (inside a torch allocation: it cannot fault)."""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def floats(self, n, name):
        buf = torch.full((n + TAIL,), float("nan"), dtype=torch.float32, device=self.dev)
        self.bufs.append((name, buf, n))
        return buf[:n]

    def doubles(self, n, name):
        buf = torch.zeros(n + TAIL, dtype=torch.float64, device=self.dev)
        buf[n:].view(torch.int64).fill_(F64_BITS)
        self.bufs.append((name, buf, n))
        return buf[:n]

    def check(self, what):
        for name, buf, n in self.bufs:
            if buf.dtype == torch.float32:
                ok = bool((buf[n:].view(torch.int32) == NAN_BITS).all())
            else:
                ok = bool((buf[n:].view(torch.int64) == F64_BITS).all())
            assert ok, "%s: the library wrote behind the %d elements of `%s`" % (what, n, name)


def _nhwc(t):
    """the physical [N, H, W, C] memory of an activation, unambiguous also for one channel or one pixel"""
    return t.permute(0, 2, 3, 1).contiguous()


def _ws_query(lib, op, case):
    nfl = int(lib.raw("mvs_conv2d_workspace_floats", op, case.n, case.hw[0], case.hw[1], case.cin, case.cout, case.ks, case.stride))
    assert nfl > 0, "%s: workspace query says %d" % (case.id, nfl)
    return nfl


def batch_ws_query(case, lib):
    """(mvs_conv2d_wgrad_batch_workspace_floats under the knobs in force, the shapes as the C array the calls take)"""
    import ctypes as C
    shapes = []
    for cin, cout, ks, hw, wcl, xf in case.opt["layers"]:
        shapes += [case.n, hw[0], hw[1], cin, cout, ks, 2 if ks == 5 else 1, int(wcl)]
    arr = (C.c_int * len(shapes))(*shapes)
    return int(lib.raw("mvs_conv2d_wgrad_batch_workspace_floats", len(case.opt["layers"]), arr)), arr


def run_owned(case, inp, lib, v, what=""):
    """The same call through lib.call with every written buffer owned by the test: outputs pre-filled with NaN, the workspace at
    EXACTLY the size the query returned (under the variant's knobs), 1024 canary elements behind each.  -> {"out", "slots"}; asserts the
    canaries and that every output element was written."""
    from mvs_amd import ops
    import ctypes as C
    dev = (inp["xs"][0] if case.op == "wgrad_batch" else inp["w"]).device
    can = Canaries(dev)
    st = ops._stream(torch.empty(0, device=dev))
    groups = case.opt.get("groups", 1)
    what = what or "%s/%s" % (case.id, v.name)
    if case.op == "wgrad_batch":
        lays = case.opt["layers"]
        xs, gys = [_nhwc(t) for t in inp["xs"]], [_nhwc(t) for t in inp["gys"]]
        nfl, arr = batch_ws_query(case, lib)
        assert nfl > 0, what
        assert nfl == v.opts.get("ws_floats", nfl), "%s: the plan asks for %d floats, the work split of the case table for %d" % (what, nfl, v.opts["ws_floats"])
        ws = can.floats(nfl, "ws")
        flat = [can.floats(cout * cin * ks * ks, "gw[%d]" % i) for i, (cin, cout, ks, _, _, _) in enumerate(lays)]
        if any(t is not None for t in inp["x_stats"]):
            sp = (C.c_void_p * len(lays))()
            for i, t in enumerate(inp["x_stats"]):
                if t is not None:
                    sp[i] = t.data_ptr()
            lib.call("mvs_conv2d_wgrad_batch_xf", len(lays), ops._ptr_array(xs), sp, case.n // groups, ops._ptr_array(gys), ops._ptr_array(flat),
                     ops._p(ws), arr, st)
        else:
            lib.call("mvs_conv2d_wgrad_batch", len(lays), ops._ptr_array(xs), ops._ptr_array(gys), ops._ptr_array(flat), ops._p(ws), arr, st)
        outs = [f.view(cout, ks, ks, cin).permute(0, 3, 1, 2) if wcl else f.view(cout, cin, ks, ks) for f, (cin, cout, ks, _, wcl, _) in zip(flat, lays)]
        res = {"out": outs, "slots": None}
    else:
        n, (h, w_), cin, cout, ks, stride = case.n, case.hw, case.cin, case.cout, case.ks, case.stride
        ho, wo = out_hw(case.hw, stride)
        wcl = 1 if v.opts.get("wcl") else 0
        wt = inp["w"].permute(0, 2, 3, 1).contiguous() if wcl else inp["w"].contiguous()
        if case.op in ("fwd", "stats", "xf"):
            x = _nhwc(inp["x"])
            ws = can.floats(_ws_query(lib, 0, case), "ws")
            y = can.floats(n * ho * wo * cout, "y")
            slots = None
            if case.op == "fwd":
                bias = inp.get("bias")
                if case.opt.get("slope") is not None:
                    lib.call("mvs_conv2d_lrelu_fwd", ops._p(x), ops._p(wt), ops._p(bias), ops._p(y), ops._p(ws), n, h, w_, cin, cout, ks, stride,
                             float(case.opt["slope"]), st)
                else:
                    lib.call("mvs_conv2d_fwd_wl", ops._p(x), ops._p(wt), ops._p(bias), ops._p(y), ops._p(ws), n, h, w_, cin, cout, ks, stride, wcl, st)
            else:
                nslots = case.opt["nslots"]
                slots = can.doubles(groups * nslots * 2 * cout, "slots")
                packed = 1 if v.opts.get("packed") else 0
                if packed:
                    lib.call("mvs_conv2d_pack_weights_batch", 1, ops._ptr_array([wt]), ops._ptr_array([ws]), (C.c_int * 4)(cin, cout, ks, stride),
                             (C.c_int * 1)(wcl), st)
                elif wcl:
                    raise ValueError("mvs_conv2d_fwd_stats reads a contiguous parameter unless the image is packed ahead")
                if case.op == "xf":
                    lib.call("mvs_conv2d_fwd_stats_xf", ops._p(x), ops._p(inp["in_stats"]), ops._p(wt), ops._p(y), ops._p(ws), ops._p(slots), nslots,
                             groups, n, h, w_, cin, cout, ks, stride, packed, st)
                else:
                    lib.call("mvs_conv2d_fwd_stats", ops._p(x), ops._p(wt), ops._p(y), ops._p(ws), ops._p(slots), nslots, groups, n, h, w_, cin, cout,
                             ks, stride, packed, st)
                slots = slots.view(groups, nslots, 2, cout)
            res = {"out": y.view(n, ho, wo, cout).permute(0, 3, 1, 2), "slots": slots}
        elif case.op in ("dgrad", "bst"):
            gy = _nhwc(inp["gy"])
            ws = can.floats(_ws_query(lib, 1, case), "ws")
            gx = can.floats(n * h * w_ * cin, "gx")
            slots = None
            if case.op == "bst":
                nslots = case.opt["nslots"]
                slots = can.doubles(groups * nslots * 2 * cin, "slots")
                raw = _nhwc(inp["raw"])
                lib.call("mvs_conv2d_dgrad_bnstats", ops._p(gy), ops._p(wt), ops._p(gx), ops._p(ws), n, h, w_, cin, cout, ks, ops._p(raw),
                         ops._p(inp["stats"]), ops._p(slots), nslots, groups, st)
                slots = slots.view(groups, nslots, 2, cin)
            else:
                lib.call("mvs_conv2d_dgrad_wl", ops._p(gy), ops._p(wt), ops._p(gx), ops._p(ws), n, h, w_, cin, cout, ks, stride, wcl, st)
            res = {"out": gx.view(n, h, w_, cin).permute(0, 3, 1, 2), "slots": slots}
        else:
            x, gy = _nhwc(inp["x"]), _nhwc(inp["gy"])
            ws = can.floats(_ws_query(lib, 2, case), "ws")
            gw = can.floats(cout * cin * ks * ks, "gw")
            lib.call("mvs_conv2d_wgrad", ops._p(x), ops._p(gy), ops._p(gw), ops._p(ws), n, h, w_, cin, cout, ks, stride, st)
            res = {"out": gw.view(cout, cin, ks, ks), "slots": None}
    can.check(what)
    for t in (res["out"] if isinstance(res["out"], list) else [res["out"]]):
        # (pre-filled with NaN: a pixel of a stride-2 input gradient belongs to exactly one parity class, and the early return of the
        #  one-pass kernel must not skip a live tile)
        assert bool(torch.isfinite(t).all()), "%s: %d output elements were never written" % (what, int((~torch.isfinite(t)).sum()))
    return res


# ---- criteria shared by the emulation and the GPU test ---------------------------------------------------------------------------
def error_row(ours, ref32, truth64):
    t = truth64.float()
    e_o, e_r = (ours - t).abs(), (ref32 - t).abs()
    return {"max_err": float(e_o.max()), "max_err_fp32": float(e_r.max()), "mean_err": float(e_o.mean()), "mean_err_fp32": float(e_r.mean())}


def absolute_bound(case, truth):
    """test_conv2d_family_vs_torch's bounds: 3e-4 forward, 5e-4 input gradient, 1e-3 x max(1, |gw|max) weight gradient"""
    if case.op in ("wgrad", "wgrad_batch"):
        return 1e-3 * max(1.0, float(truth.abs().max()))
    return 5e-4 if case.op in ("dgrad", "bst") else 3e-4


def report(row):
    """one JSON line per case and variant into the file MVS_ARM_REPORT names (or conv2d_arm_parity_ratios.jsonl next to
    MVS_GRAD_REPORT's file, when only that is set); the copy kept with the project is profiles/conv2d_arm_parity_ratios.jsonl"""
    out = os.environ.get("MVS_ARM_REPORT", "")
    if out:
        out = os.path.join(os.path.dirname(os.path.abspath(out)), "conv2d_arm_parity_ratios.jsonl")
    elif os.environ.get("MVS_GRAD_REPORT"):
        out = os.path.join(os.path.dirname(os.path.abspath(os.environ["MVS_GRAD_REPORT"])), "conv2d_arm_parity_ratios.jsonl")
    if not out:
        return
    try:
        with open(out, "a") as fh:
            fh.write(json.dumps(row) + "\n")
    except OSError:
        pass


def check_numbers(case, lib, dev, calls, record=None):
    """The criteria of a case, shared with the GPU test.  calls(case, inp, lib, v) -> [result, ...]: the calls of variant v (each
    {"out", "slots"}) -- all of them must agree bit for bit on the output (no float atomics there; the deterministic finish covers the
    reduces); the first is compared with the references."""
    from mvs_amd import ops
    from conftest import assert_as_accurate_as_fp32_reference, assert_grads_as_accurate_as_fp32_reference
    inp = make_inputs(case)
    t64, r32 = reference(case, inp, torch.float64), reference(case, inp, torch.float32)
    dinp = to_device(inp, dev)
    many = isinstance(t64["out"], list)
    as_list = lambda o: [t.cpu() for t in o] if many else [o.cpu()]
    truth, yard = as_list(t64["out"]), as_list(r32["out"])
    got = {}
    for v in case.variants:
        what = "%s/%s" % (case.id, v.name)
        with lib.tuning(**v.knobs):
            lib.launch_trace()
            results = calls(case, dinp, lib, v)
            trace = lib.launch_trace()
            assert trace == v.trace * len(results), "%s took %s" % (what, trace)
            outs = [as_list(r["out"]) for r in results]
            for o in outs[1:]:
                for a, b in zip(outs[0], o):
                    assert torch.equal(a, b), "%s: two calls differ by %.3e" % (what, float((a - b).abs().max()))
            if case.op in ("stats", "xf"):
                # y must be the plain kernel's, bit for bit.  XF: the plain kernel on relu(x * scale + shift) written out by torch in
                # fp32 (a multiply, then an add: the staging's arithmetic) -- the same values enter the same MFMA chain
                xin = _normalised(dinp["x"], dinp["in_stats"], torch.float32).contiguous(memory_format=CL) if case.op == "xf" else dinp["x"]
                plain = ops.conv2d_forward(xin, dinp["w"], None, case.stride)
                lib.launch_trace()
                assert torch.equal(outs[0][0], plain.cpu()), "%s: y differs from the plain kernel's" % what
        got[v.name] = outs[0]
        rows = [error_row(o, y, t) for o, y, t in zip(outs[0], yard, truth)]
        row = {k: max(r[k] for r in rows) for k in rows[0]}
        row.update(case=case.id, variant=v.name, op=case.op, trace=trace[:len(v.trace)], slack_allowed=4.0)
        # accuracy: the project's criterion (conftest, default slack 4) + the family test's absolute bounds
        if case.op in ("wgrad", "wgrad_batch"):
            names = ["gw%d" % i for i in range(len(truth))]
            assert_grads_as_accurate_as_fp32_reference(dict(zip(names, outs[0])), dict(zip(names, yard)), dict(zip(names, truth)), what=what)
        else:
            assert_as_accurate_as_fp32_reference(outs[0][0], yard[0], truth[0], what=what)
        for o, t, r in zip(outs[0], truth, rows):
            assert r["max_err"] < absolute_bound(case, t), "%s: max err %.3e over the family test's bound %.1e" % (what, r["max_err"], absolute_bound(case, t))
        # statistic slots
        for r in results:
            if case.op in ("stats", "xf"):
                # against fp64 sums of the device's own y and y^2 (test_conv2d_forward_with_batchnorm_partial_sums' tolerance)
                y = r["out"].cpu().double()
                g = r["slots"].shape[0]
                yg = y.reshape(g, case.n // g, *y.shape[1:])
                per = r["slots"].cpu().sum(1)
                assert torch.allclose(per[:, 0], yg.sum(dim=(1, 3, 4)), rtol=1e-4, atol=1e-3), "%s: sum(y) slots" % what
                assert torch.allclose(per[:, 1], (yg * yg).sum(dim=(1, 3, 4)), rtol=1e-4, atol=1e-3), "%s: sum(y^2) slots" % what
            elif case.op == "bst":
                # against the fp64 reference's sums; the yardstick is the error of the fp32 CPU reference's sums on the same inputs
                per = r["slots"].cpu().sum(1)
                e_o = float((per - t64["stats"]).abs().max())
                e_r = float((r32["stats"].double() - t64["stats"]).abs().max())
                row.update(bst_sums_err=e_o, bst_sums_err_fp32=e_r)
                assert e_o <= 4.0 * e_r + 2e-6, "%s: backward sums err %.3e vs fp32 reference err %.3e (ratio %.2f)" % (what, e_o, e_r, e_o / max(e_r, 1e-300))
        print("%s: %s" % (what, row))
        if record is not None:
            record(row)
    # knob pairs / call forms on identical inputs
    for a, b, kind in case.pairs:
        for x, y, t in zip(got[a], got[b], truth):
            if kind == "equal":
                assert torch.equal(x, y), "%s: %s and %s differ by %.3e" % (case.id, a, b, float((x - y).abs().max()))
            else:
                scale = max(1.0, float(t.abs().max()))
                assert float((x - y).abs().max()) < 2e-4 * scale, "%s: %s vs %s: %.3e" % (case.id, a, b, float((x - y).abs().max()))
