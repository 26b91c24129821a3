// The measurement knobs (mvs_set_tuning / mvs_get_tuning, include/mvs_hip.h): THE list.  One row per knob -- key, default, lowest and
// highest accepted value (a set clamps to them), meaning.  The key is also the field name: a launcher reads g_tune.<key>.  The
// struct, its defaults and the name table of mvs_common.cpp are generated from this list; _lib.DEFAULT_TUNING mirrors some of the
// defaults and tests/test_capi_symbols.py holds it against a freshly loaded library.
// The one piece of process-wide mutable state of the library: host variables that the launchers read unsynchronised, to be changed
// only while no other thread is inside the library.  They choose between kernels (A/B runs of bench.py and tools/, the tests of the
// size-selected variants); they are not part of the data path's contract.  The measurements behind a default stand where the
// knob is read.
#pragma once

#define MVS_KNOBS(X) \
    /* plane sweep (plane_sweep.hip) */ \
    X(nt,               0,    0, 1,       "forward: non-temporal stores of the variance volume") \
    X(tile_w,           0,    0, 256,     "cached forward: pixel-tile width, 0 = the default tile") \
    X(dslab,            0,    0, 1 << 20, "forward: planes per workgroup, 0 = auto") \
    X(sweep_fwd,        3,    0, 4,       "forward: 0 taps through L1 every plane, 1 LDS-staged windows, 2 register-cached taps (4 ch/thread), 3 (8 ch/thread), 4 (16 ch/thread, <= 2 source views)") \
    X(sweep_bwd,        0,    0, 1,       "backward: 0 per-wave windows (<= 4 source views), 1 view-pair kernel with LDS atomics (what > 4 source views run)") \
    X(bwd_dslab,        0,    0, 1 << 20, "per-wave-window backward: planes per workgroup, 0 = auto") \
    X(bwd_nowin,        0,    0, 1,       "(tests) 1 = no LDS windows, every flush through global atomics") \
    X(bwd_cpt,          4,    4, 8,       "accepted and ignored (the 8-channels-per-thread backward was measured slower and removed)") \
    X(bwd_pf,           0,    0, 2,       "backward: 1 = block lookahead for 1-2 source views, 2 = ONE wave per SIMD for 3-4 source views") \
    X(bwd_gd,           2,    0, 2,       "backward: 2 = upstream gradient requested two planes ahead at 2 waves/SIMD (1-2 source views), 0 = rotating set at 3 waves/SIMD") \
    X(bwd_gd34,         0,    0, 1,       "backward: 3-4 source views with the upstream gradient requested two planes ahead (as 1-2 views run), 2 waves/SIMD") \
    X(fwd_pt,           0,    0, 1,       "cached forward with the per-wave projection table (plane_sweep_variance_fwd_pt_kernel): measured and rejected") \
    X(bwd_gpf,          0,    0, 1,       "per-wave-window backward requests the next planes' upstream gradient: 0 top of the group, 1 after the plane's gathers") \
    X(fwd_dl,           2,    0, 2,       "forward: 0 the round-1 loop, 1 LDS-staged per-plane depths, 2 + all views' re-gathers in flight before the first sample") \
    X(sweep_xcd,        0,    0, 1,       "XCD-compact workgroup order of the cached forward and the per-wave-window backward") \
    /* 3-D convolutions (conv3d.hip, conv3d_pers.hip, conv3d_x3.hip, conv3d_bf16.hip) */ \
    X(conv_split,       1,    0, 1,       "0 keeps all Cout tiles in one workgroup") \
    X(conv_small,       1,    0, 2,       "quarter-size workgroup tiles for under-filled launches (0 never, 1 auto, 2 always)") \
    X(conv_small_wgs,   384,  0, 1 << 20, "... below this many workgroups (~1.5 per CU)") \
    X(tr2pw,            1,    0, 1,       "transposed stride-2 conv with Cout == 8 as W-parity-merged GEMMs (GEOM_TR2_PW)") \
    X(cc_wide,          0,    0, 1,       "quarter-tile kernels of the deep levels with all input channels as one chunk: measured and rejected") \
    X(cin1_vpt,         1,    1, 5,       "voxels per thread of the Cout == 1 layer's input gradient (4 = four from 1 M voxels on, 5 = always four): measured and rejected") \
    X(k8,               7,    0, 15,      "bit mask: 1|2 = Cout == 8 stride-1 layers run the 4x4x1 MFMA forward with the weights as the broadcast operand (0: generic kernel), +4 = weight gradient with g as the broadcast operand") \
    X(cout1_d4,         2,    0, 3,       "bit 1: the Cout = 1 layer of the bf16 inference path with four outputs per thread") \
    X(cout1_h4,         1,    0, 1,       "the 8 -> 1 layer with four outputs per thread (conv_cout1_h4_kernel); 0: one output per thread") \
    X(bf16_dp,          1,    0, 1,       "conv0 of the bf16 path (32 -> 8) with two output depth slices per MFMA (GEOM_S1_DP)") \
    X(xcd,              1,    0, 1,       "XCD-aware tile order in the broadcast-operand forward and the Cout == 8 weight gradient") \
    X(side_pre,         1,    0, 1,       "one-Cout-tile kernels with epilogue side inputs (skip / bn_raw) request them before the k-loop (1) or at the top of the epilogue (0)") \
    X(conv_pers,        1,    0, 1,       "one-chunk layers (16 -> <= 16, 8 -> 32 stride 1; 8 -> <= 16 stride 2) run the persistent kernels of conv3d_pers.hip") \
    X(conv_pers_min,    1024, 0, 1 << 30, "... when the one-tile kernel would launch at least this many workgroups (a persistent grid needs several tiles per workgroup)") \
    X(conv_pers_groups, 0,    0, 4096,    "workgroups of a persistent launch, 0 = what fits the GPU (tests: a few workgroups walk many tiles)") \
    X(conv_pers_nw,     8,    4, 8,       "waves per workgroup of conv_pers_kernel") \
    X(wgrad_pers,       1,    0, 1,       "one-chunk weight gradients run conv3d_pers.hip, from conv_pers_min tiles on") \
    X(wgrad_small,      0,    0, 3,       "quarter-size tiles in the generic weight-gradient kernel: 1 = 8-channel / stride-2 layers with many tiles, 2 = every layer with many tiles, 3 = always (tests)") \
    X(wgrad_groups,     768,  1, 768,     "persistent workgroups of the generic weight-gradient kernels") \
    X(wgrad8_groups,    192,  1, 512,     "... of the CG == 8 kernel (conv0)") \
    X(wgrad8_gs,        2,    0, 2,       "conv0's weight gradient in the output-gradient-shifted form on the 16x16x4 MFMA (conv_c8_wgrad_gs_kernel): 1 eight waves per workgroup, 2 sixteen; 0: conv_c8_wgrad_kernel (4x4x1 MFMA, X shifted)") \
    X(wgrad8_nch,       2,    1, 2,       "2 = the CG == 8 weight gradient stages both 16-channel chunks of a 32-channel X in one workgroup") \
    X(conv0_x3,         0,    0, 3,       "split-bf16 products (conv3d_x3.hip, opt-in): bit 0 = conv0's input gradient, bit 1 = conv0's forward") \
    /* 2-D convolutions (conv2d.hip) */ \
    X(conv2d_pp,        1,    0, 1,       "3x3 stride-1 layers with <= 8 output channels as pixel-pair GEMMs (conv2d_igemm_kernel<.., PP>)") \
    X(conv2d_s2_mfma,   2,    0, 2,       "stride-2 input gradient: 2 ONE four-class MFMA pass with compacted taps, 1 four parity-class passes, 0 direct VALU form") \
    X(wgrad2d_groups,   256,  0, 1 << 20, "persistent workgroups of the weight gradient (used: 1 .. 1024; 256 = one per CU)") \
    X(wgrad2d_batch,    2048, 1, 4096,    "workgroups of the batched weight gradient (both launches together), shared out by work") \
    /* wide forward 2-D convolutions of the frozen trunk (conv2d_wide_kernels.h) */ \
    X(c2w_tile,         0,    0, 2,       "0 = t128x64 when its launch has at least c2w_big_min workgroups, else t64x64; 1 = always t64x64; 2 = always t128x64") \
    X(c2w_big_min,      512,  0, 1 << 30, "... workgroups (two per CU)") \
    X(c2w_splitk,       0,    0, 8,       "K ranges of a layer: 0 = doubled (<= 8) while a t64x64 launch has fewer than c2w_split_min workgroups, 1 = never split, 2..8 = this many") \
    X(c2w_split_min,    512,  0, 1 << 30, "... workgroups (two per CU)") \
    X(c2w_bf_split_min, 2048, 0, 1 << 30, "c2w_split_min of the bf16 arms (arith = bf16): eight workgroups per CU")

struct MvsTuning {
#define MVS_KNOB_FIELD(key, def, lo, hi, doc) int key;
    MVS_KNOBS(MVS_KNOB_FIELD)
#undef MVS_KNOB_FIELD
};
extern MvsTuning g_tune;   // mvs_common.cpp
