// One C call per pass of the TRAINING 2-D feature extractor.
//
// The reference runs FeatureNet (jdacs/models/mvsnet.py:17-34: seven ConvBnReLU blocks -- 3x3 stride 1 / 5x5 stride 2, module.py:15-22 --
// closed by a plain 3x3 convolution with bias) as 15 nn.Module calls forward and ~30 autograd nodes backward.  The Python mirror
// (ops.FeatureExtractorFn) had made that ONE autograd node in round 4, but the node still issued ~17 C-ABI calls forward and ~30 backward
// from Python -- pointer extraction, ctypes marshalling, a torch allocation or three per call: ~1 ms of launch-thread time per training
// step for ~1 ms of kernels.  These two entry points are the same launch sequence (same kernels, same order, same streams) driven from C,
// in the node's default configuration:
//   * every convolution through csrc/conv2d.hip (forward with BatchNorm's statistics in its epilogue; input gradients; the one-launch
//     weight gradient of all layers),
//   * consumer-side BatchNorm: block i's relu(bn(.)) is applied by block i+1's convolution and weight gradient while they stage their
//     input; only a finalize launch per block, the LAST block's output is materialised for the closing convolution,
//   * backward: the weight gradients of the layers from `early_from` up are forked to `side` as soon as their output gradients exist
//     (behind a HIP event recorded on `main`), the rest follow on `main` at the end; `main` waits for `side` before the call returns.
// The caller hands over a table of blocks and tables of device pointers (its own allocations; nothing is allocated here).
// Every tensor is channels-last fp32 ([N,H,W,C]) as everywhere in this library.
#include <string.h>
#include "mvs_rt.h"

#define MVS_FEAT_MAX_BLOCKS 7
extern "C" {
struct MvsFeatBlock {                 // == include/mvs_hip.h
    int cin, cout, ks, stride;
    float eps, momentum;
    int w_channels_last;              // the parameter tensor is [Cout][ks][ks][Cin] in memory (a channels_last nn.Conv2d weight)
    int h, w;                         // spatial dims of the block's INPUT
};
int mvs_conv2d_fwd_wl(const float* x, const float* w, const float* bias, float* y, float* ws, int N, int H, int W, int Cin, int Cout, int ks,
                      int stride, int w_channels_last, hipStream_t stream);
int mvs_conv2d_fwd_stats(const float* x, const float* w, float* y, float* ws, double* slots, int nslots, int G, int N, int H, int W, int Cin,
                         int Cout, int ks, int stride, int ws_packed, hipStream_t stream);
int mvs_conv2d_fwd_stats_xf(const float* x, const float* in_stats, const float* w, float* y, float* ws, double* slots, int nslots, int G, int N,
                            int H, int W, int Cin, int Cout, int ks, int stride, int ws_packed, hipStream_t stream);
int mvs_conv2d_pack_weights_batch(int n, const float* const* w, float* const* ws, const int* shapes, const int* w_channels_last,
                                  hipStream_t stream);
int mvs_conv2d_dgrad_wl(const float* gy, const float* w, float* gx, float* ws, int N, int H, int W, int Cin, int Cout, int ks, int stride,
                        int w_channels_last, hipStream_t stream);
int mvs_conv2d_wgrad_batch_xf(int n, const float* const* x, const float* const* x_stats, int imgs_per_group, const float* const* gy,
                              float* const* gw, float* ws, const int* shapes, hipStream_t stream);
int mvs_conv2d_wgrad_batch(int n, const float* const* x, const float* const* gy, float* const* gw, float* ws, const int* shapes,
                           hipStream_t stream);
int mvs_bn_finalize_slots(const double* slots, int nslots, int G, long long Vg, int C, const float* gamma, const float* beta, float eps,
                          float momentum, float* running_mean, float* running_var, float* stats, hipStream_t stream);
int mvs_bn_relu_fwd_slots(const float* x, const double* slots, int nslots, int G, long long Vg, int C, const float* gamma, const float* beta,
                          float eps, float momentum, float* running_mean, float* running_var, const float* skip, int relu, float* stats,
                          float* y, hipStream_t stream);
int mvs_bn_bwd_reduce_slots(const float* dy, const float* x, const float* stats, int relu, int G, long long Vg, int C, double* slots,
                            int nslots, hipStream_t stream);
int mvs_bn_relu_bwd_slots(const float* dy, const float* x, const float* stats, const double* slots, int nslots, int relu, int G, long long Vg,
                          int C, float* dx, float* dgamma, float* dbeta, hipStream_t stream);
}

#define MVS_TRY(call)               \
    do {                            \
        const int rc_ = (call);     \
        if (rc_ != MVS_OK) return rc_; \
    } while (0)

static void out_hw(const MvsFeatBlock& b, int& ho, int& wo) {
    if (b.stride == 1) { ho = b.h; wo = b.w; }
    else { ho = (b.h - 1) / 2 + 1; wo = (b.w - 1) / 2 + 1; }
}

static int check_blocks(int n, const MvsFeatBlock* blk, int N, int G, const char* what) {
    MVS_REQUIRE(n >= 2 && n <= MVS_FEAT_MAX_BLOCKS && blk, MVS_ERR_SHAPE, "%s: 2..%d blocks, got %d", what, MVS_FEAT_MAX_BLOCKS, n);
    MVS_REQUIRE(N >= 1 && G >= 1 && N % G == 0, MVS_ERR_SHAPE, "%s: %d images do not split into %d statistics groups", what, N, G);
    for (int i = 0; i < n; ++i) {
        MVS_REQUIRE((blk[i].ks == 3 && blk[i].stride == 1) || (blk[i].ks == 5 && blk[i].stride == 2), MVS_ERR_UNSUPPORTED,
                    "%s: block %d is %dx%d stride %d (3x3 stride 1 or 5x5 stride 2)", what, i, blk[i].ks, blk[i].ks, blk[i].stride);
        if (i > 0) {
            int ho, wo;
            out_hw(blk[i - 1], ho, wo);
            MVS_REQUIRE(blk[i].cin == blk[i - 1].cout && blk[i].h == ho && blk[i].w == wo, MVS_ERR_SHAPE,
                        "%s: block %d does not read block %d's output", what, i, i - 1);
        }
    }
    return MVS_OK;
}

extern "C" int mvs_feature_fwd(int n, const MvsFeatBlock* blk, int N, int G, const float* x, const float* const* w, const float* const* gamma,
                               const float* const* beta, float* const* running_mean, float* const* running_var, float* const* packed,
                               float* const* raw, float* y_last, float* const* stats, double* const* slots, const int* nslots,
                               const float* wclose, const float* bclose, int close_cout, int close_w_channels_last, float* ws_close, float* out,
                               hipStream_t stream) {
    MVS_TRY(check_blocks(n, blk, N, G, "mvs_feature_fwd"));
    MVS_REQUIRE(x && w && gamma && beta && running_mean && running_var && packed && raw && y_last && stats && slots && nslots && wclose &&
                ws_close && out, MVS_ERR_NULL, "mvs_feature_fwd: null pointer argument");
    int shapes[4 * MVS_FEAT_MAX_BLOCKS], wcl[MVS_FEAT_MAX_BLOCKS];
    for (int i = 0; i < n; ++i) {
        shapes[4 * i] = blk[i].cin; shapes[4 * i + 1] = blk[i].cout; shapes[4 * i + 2] = blk[i].ks; shapes[4 * i + 3] = blk[i].stride;
        wcl[i] = blk[i].w_channels_last;
    }
    MVS_TRY(mvs_conv2d_pack_weights_batch(n, w, packed, shapes, wcl, stream));      // the forward weight images of all blocks: ONE launch
    int ho = 0, wo = 0;
    for (int i = 0; i < n; ++i) {
        const MvsFeatBlock& b = blk[i];
        if (i == 0)
            MVS_TRY(mvs_conv2d_fwd_stats(x, w[i], raw[i], packed[i], slots[i], nslots[i], G, N, b.h, b.w, b.cin, b.cout, b.ks, b.stride, 1, stream));
        else     // the block in front is applied while this convolution stages its input
            MVS_TRY(mvs_conv2d_fwd_stats_xf(raw[i - 1], stats[i - 1], w[i], raw[i], packed[i], slots[i], nslots[i], G, N, b.h, b.w, b.cin, b.cout,
                                            b.ks, b.stride, 1, stream));
        out_hw(b, ho, wo);
        const long long vg = (long long)(N / G) * ho * wo;
        if (i < n - 1)
            MVS_TRY(mvs_bn_finalize_slots(slots[i], nslots[i], G, vg, b.cout, gamma[i], beta[i], b.eps, b.momentum, running_mean[i],
                                          running_var[i], stats[i], stream));
        else
            MVS_TRY(mvs_bn_relu_fwd_slots(raw[i], slots[i], nslots[i], G, vg, b.cout, gamma[i], beta[i], b.eps, b.momentum, running_mean[i],
                                          running_var[i], nullptr, 1, stats[i], y_last, stream));
    }
    return mvs_conv2d_fwd_wl(y_last, wclose, bclose, out, ws_close, N, ho, wo, blk[n - 1].cout, close_cout, 3, 1, close_w_channels_last, stream);
}

#if defined(MVS_CPU_EMUL)
static void fork_event(hipStream_t, hipStream_t) {}
#else
static void fork_event(hipStream_t from, hipStream_t to) {
    static thread_local hipEvent_t ev = nullptr;
    if (!ev) (void)hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    (void)hipEventRecord(ev, from);
    (void)hipStreamWaitEvent(to, ev, 0);
}
#endif

// layers lo .. hi-1 of the chain (layer n = the closing convolution) as one weight-gradient batch on `st`
static int wgrad_range(int n, const MvsFeatBlock* blk, int N, int G, int close_cout, int close_wcl, int lo, int hi, const float* x,
                       const float* const* raw, const float* y_last, const float* const* stats, float* const* draw, const float* gout,
                       float* const* gw, float* ws, hipStream_t st) {
    const float* xs[MVS_FEAT_MAX_BLOCKS + 1];
    const float* xst[MVS_FEAT_MAX_BLOCKS + 1];
    const float* gys[MVS_FEAT_MAX_BLOCKS + 1];
    float* gws[MVS_FEAT_MAX_BLOCKS + 1];
    int shapes[8 * (MVS_FEAT_MAX_BLOCKS + 1)];
    bool any_stats = false;
    int cnt = 0;
    for (int j = lo; j < hi; ++j, ++cnt) {
        // the input of layer j: the images (j = 0), the RAW output of block j-1 normalised while staged (0 < j < n), the materialised
        // output of the last block (the closing convolution)
        xs[cnt] = j == 0 ? x : (j == n ? y_last : raw[j - 1]);
        xst[cnt] = (j > 0 && j < n) ? stats[j - 1] : nullptr;
        any_stats = any_stats || xst[cnt] != nullptr;
        gys[cnt] = j == n ? gout : draw[j];
        gws[cnt] = gw[j];
        int* s = shapes + 8 * cnt;
        if (j < n) {
            s[0] = N; s[1] = blk[j].h; s[2] = blk[j].w; s[3] = blk[j].cin; s[4] = blk[j].cout; s[5] = blk[j].ks; s[6] = blk[j].stride;
            s[7] = blk[j].w_channels_last;
        } else {
            int ho, wo;
            out_hw(blk[n - 1], ho, wo);
            s[0] = N; s[1] = ho; s[2] = wo; s[3] = blk[n - 1].cout; s[4] = close_cout; s[5] = 3; s[6] = 1; s[7] = close_wcl;
        }
    }
    if (cnt == 0) return MVS_OK;
    if (any_stats) return mvs_conv2d_wgrad_batch_xf(cnt, xs, xst, N / G, gys, gws, ws, shapes, st);
    return mvs_conv2d_wgrad_batch(cnt, xs, gys, gws, ws, shapes, st);
}

extern "C" int mvs_feature_bwd(int n, const MvsFeatBlock* blk, int N, int G, const float* x, const float* const* w, const float* wclose,
                               int close_cout, int close_w_channels_last, const float* const* raw, const float* y_last,
                               const float* const* stats, double* const* slots_b, const int* nslots, const float* gout, float* const* gbuf,
                               float* const* draw, float* gx, float* dgrad_ws, float* const* gw, float* wgrad_ws_main, float* wgrad_ws_side,
                               float* const* dgamma, float* const* dbeta, int early_from, hipStream_t main_stream, hipStream_t side_stream,
                               int* side_stream_used) {
    MVS_TRY(check_blocks(n, blk, N, G, "mvs_feature_bwd"));
    MVS_REQUIRE(x && w && wclose && raw && y_last && stats && slots_b && nslots && gout && gbuf && draw && dgrad_ws && gw && wgrad_ws_main &&
                dgamma && dbeta, MVS_ERR_NULL, "mvs_feature_bwd: null pointer argument");
    for (int j = 0; j <= n; ++j) MVS_REQUIRE(gw[j], MVS_ERR_NULL, "mvs_feature_bwd: every layer's weight gradient is computed (gw[%d] is null)", j);
    const bool async = side_stream != nullptr && side_stream != main_stream && early_from > 0 && early_from < n && wgrad_ws_side != nullptr;
    bool side_used = false;
    struct Closer {       // a failure after the fork must not leave work on the side stream unjoined
        bool& used; hipStream_t side, main; int* out;
        ~Closer() { if (used) fork_event(side, main); if (out) *out = used ? 1 : 0; }
    } closer{side_used, side_stream, main_stream, side_stream_used};
    int ho, wo;
    out_hw(blk[n - 1], ho, wo);
    // the closing convolution's input gradient = the output gradient of the last block
    MVS_TRY(mvs_conv2d_dgrad_wl(gout, wclose, gbuf[n - 1], dgrad_ws, N, ho, wo, blk[n - 1].cout, close_cout, 3, 1, close_w_channels_last,
                                main_stream));
    for (int i = n - 1; i >= 0; --i) {
        const MvsFeatBlock& b = blk[i];
        out_hw(b, ho, wo);
        const long long vg = (long long)(N / G) * ho * wo;
        MVS_TRY(mvs_bn_bwd_reduce_slots(gbuf[i], raw[i], stats[i], 1, G, vg, b.cout, slots_b[i], nslots[i], main_stream));
        MVS_TRY(mvs_bn_relu_bwd_slots(gbuf[i], raw[i], stats[i], slots_b[i], nslots[i], 1, G, vg, b.cout, draw[i], dgamma[i], dbeta[i],
                                      main_stream));
        if (async && i == early_from) {
            fork_event(main_stream, side_stream);         // draw[early_from .. n-1] and gout exist on the main stream
            side_used = true;
            MVS_TRY(wgrad_range(n, blk, N, G, close_cout, close_w_channels_last, early_from, n + 1, x, raw, y_last, stats, draw, gout, gw,
                                wgrad_ws_side, side_stream));
        }
        if (i > 0)
            MVS_TRY(mvs_conv2d_dgrad_wl(draw[i], w[i], gbuf[i - 1], dgrad_ws, N, b.h, b.w, b.cin, b.cout, b.ks, b.stride, b.w_channels_last,
                                        main_stream));
        else if (gx)
            MVS_TRY(mvs_conv2d_dgrad_wl(draw[i], w[i], gx, dgrad_ws, N, b.h, b.w, b.cin, b.cout, b.ks, b.stride, b.w_channels_last, main_stream));
    }
    MVS_TRY(wgrad_range(n, blk, N, G, close_cout, close_w_channels_last, 0, async ? early_from : n + 1, x, raw, y_last, stats, draw, gout, gw,
                        wgrad_ws_main, main_stream));
    return MVS_OK;          // (the Closer joins side -> main and reports)
}

// ---- RefineNet (jdacs/models/mvsnet.py:77-92) as one C call per pass ---------------------------------------------------------------
// image [B,3,H,W] (any batch stride) + depth [B,h,w], h = H/4, w = W/4 -> x0 [B,h,w,4] (refine_kernels.h) -> ConvBnReLU 4 -> 32 -> 32
// -> 32 -> 1 -> depth + relu(bn(.)).  Blocks 0 and 1 are normalised by their consumers while those stage their input (as in
// mvs_feature_fwd); block 2's output y2 is materialised for the 32 -> 1 convolution, whose epilogue sums the one-channel statistics
// the tail finishes.  frozen != 0: every block normalises with its running statistics (mvs_bn_frozen_stats); nothing writes them.
extern "C" {
int mvs_conv2d_wgrad(const float* x, const float* gy, float* gw, float* ws, int N, int H, int W, int Cin, int Cout, int ks, int stride,
                     hipStream_t stream);
int mvs_conv2d_relu_fwd_packed(const float* x, float* packed, const float* bias, float* y, int N, int H, int W, int Cin, int Cout,
                               hipStream_t stream);
int mvs_bn_frozen_stats(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps, int C,
                        float* stats, hipStream_t stream);
int mvs_bn_relu_fwd(const float* x, const float* scale, const float* shift, const float* skip, int relu, long long V, int C, float* y,
                    hipStream_t stream);
int mvs_bn_relu_bwd_frozen(const float* dy, const float* raw, const float* stats, double* slots, int nslots, int have_sums, int relu,
                           long long V, int C, float* draw, float* dgamma, float* dbeta, hipStream_t stream);
int mvs_refine_assemble(const float* img, long long img_batch_stride, const float* depth, float* x0, int B, int H, int W, int h, int w,
                        hipStream_t stream);
int mvs_refine_assemble_bwd(const float* gx0, const float* gy, float* gimg, float* gdepth, int B, int H, int W, int h, int w,
                            hipStream_t stream);
int mvs_refine_tail_fwd(const float* raw, const float* depth, const double* slots, int nslots, long long V, const float* gamma,
                        const float* beta, float eps, float momentum, float* running_mean, float* running_var, float* stats, float* y,
                        hipStream_t stream);
int mvs_refine_tail_fwd_frozen(const float* raw, const float* depth, const float* stats, const float* beta, long long V, float* y,
                               hipStream_t stream);
int mvs_refine_tail_bwd(const float* gy, const float* raw, const float* stats, const float* beta, int frozen, long long V, double* rec,
                        float* draw, float* dgamma, float* dbeta, hipStream_t stream);
int mvs_refine_tail_eval(const float* x, const float* w, const float* bias, const float* depth, float* y, int B, int h, int w_,
                         hipStream_t stream);
}

static const int REFINE_CIN[4] = {4, 32, 32, 32}, REFINE_COUT[4] = {32, 32, 32, 1};

static int refine_ptrs4(const char* what, const void* const* p, const char* name) {
    MVS_REQUIRE(p, MVS_ERR_NULL, "%s: null pointer argument (%s)", what, name);
    for (int i = 0; i < 4; ++i) MVS_REQUIRE(p[i], MVS_ERR_NULL, "%s: %s[%d] is null", what, name, i);
    return MVS_OK;
}
#define REFINE_P4(what, p) MVS_TRY(refine_ptrs4(what, (const void* const*)(p), #p))

extern "C" int mvs_refine_fwd(int frozen, int B, int H, int W, int h, int wd, const float* img, long long img_batch_stride, const float* depth,
                              const float* const* w, const float* const* gamma, const float* const* beta, float* const* running_mean,
                              float* const* running_var, const float* eps, const float* momentum, float* x0, float* const* packed,
                              float* const* raw, float* y2, float* const* stats, double* const* slots, const int* nslots, float* out,
                              hipStream_t stream) {
    MVS_REQUIRE(img && depth && eps && momentum && x0 && y2 && nslots && out, MVS_ERR_NULL, "mvs_refine_fwd: null pointer argument");
    REFINE_P4("mvs_refine_fwd", w); REFINE_P4("mvs_refine_fwd", gamma); REFINE_P4("mvs_refine_fwd", beta);
    REFINE_P4("mvs_refine_fwd", running_mean); REFINE_P4("mvs_refine_fwd", running_var); REFINE_P4("mvs_refine_fwd", packed);
    REFINE_P4("mvs_refine_fwd", raw); REFINE_P4("mvs_refine_fwd", stats); REFINE_P4("mvs_refine_fwd", slots);
    MVS_TRY(mvs_refine_assemble(img, img_batch_stride, depth, x0, B, H, W, h, wd, stream));
    const long long V = (long long)B * h * wd;
    int shapes[16], wcl[4] = {0, 0, 0, 0};
    for (int i = 0; i < 4; ++i) { shapes[4 * i] = REFINE_CIN[i]; shapes[4 * i + 1] = REFINE_COUT[i]; shapes[4 * i + 2] = 3; shapes[4 * i + 3] = 1; }
    MVS_TRY(mvs_conv2d_pack_weights_batch(4, w, packed, shapes, wcl, stream));
    if (frozen)
        for (int i = 0; i < 4; ++i)
            MVS_TRY(mvs_bn_frozen_stats(gamma[i], beta[i], running_mean[i], running_var[i], eps[i], REFINE_COUT[i], stats[i], stream));
    for (int i = 0; i < 3; ++i) {
        if (i == 0)
            MVS_TRY(mvs_conv2d_fwd_stats(x0, w[0], raw[0], packed[0], slots[0], nslots[0], 1, B, h, wd, 4, 32, 3, 1, 1, stream));
        else
            MVS_TRY(mvs_conv2d_fwd_stats_xf(raw[i - 1], stats[i - 1], w[i], raw[i], packed[i], slots[i], nslots[i], 1, B, h, wd, 32, 32, 3, 1, 1,
                                            stream));
        if (frozen) continue;
        if (i < 2)
            MVS_TRY(mvs_bn_finalize_slots(slots[i], nslots[i], 1, V, 32, gamma[i], beta[i], eps[i], momentum[i], running_mean[i], running_var[i],
                                          stats[i], stream));
        else
            MVS_TRY(mvs_bn_relu_fwd_slots(raw[2], slots[2], nslots[2], 1, V, 32, gamma[2], beta[2], eps[2], momentum[2], running_mean[2],
                                          running_var[2], nullptr, 1, stats[2], y2, stream));
    }
    if (frozen) MVS_TRY(mvs_bn_relu_fwd(raw[2], stats[2] + 64, stats[2] + 96, nullptr, 1, V, 32, y2, stream));
    MVS_TRY(mvs_conv2d_fwd_stats(y2, w[3], raw[3], packed[3], slots[3], nslots[3], 1, B, h, wd, 32, 1, 3, 1, 1, stream));
    if (frozen) return mvs_refine_tail_fwd_frozen(raw[3], depth, stats[3], beta[3], V, out, stream);
    return mvs_refine_tail_fwd(raw[3], depth, slots[3], nslots[3], V, gamma[3], beta[3], eps[3], momentum[3], running_mean[3], running_var[3],
                               stats[3], out, stream);
}

// eval mode without a gradient: BatchNorm folded into the weights by the caller.  packed[3]: the forward weight images of the three
// 32-channel blocks (mvs_conv2d_pack_weights_batch of the FOLDED weights, kept by the caller while the parameters do not change),
// bias[3] their folded biases; wtail [1][32][3][3] / btail [1]: the folded 32 -> 1 layer.  5 launches.
extern "C" int mvs_refine_eval_fwd(int B, int H, int W, int h, int wd, const float* img, long long img_batch_stride, const float* depth, float* const* packed,
                                   const float* const* bias, const float* wtail, const float* btail, float* x0, float* buf_a, float* buf_b,
                                   float* out, hipStream_t stream) {
    MVS_REQUIRE(img && depth && packed && bias && wtail && btail && x0 && buf_a && buf_b && out, MVS_ERR_NULL,
                "mvs_refine_eval_fwd: null pointer argument");
    for (int i = 0; i < 3; ++i) MVS_REQUIRE(packed[i] && bias[i], MVS_ERR_NULL, "mvs_refine_eval_fwd: null weight image / bias of block %d", i);
    MVS_TRY(mvs_refine_assemble(img, img_batch_stride, depth, x0, B, H, W, h, wd, stream));
    MVS_TRY(mvs_conv2d_relu_fwd_packed(x0, packed[0], bias[0], buf_a, B, h, wd, 4, 32, stream));
    MVS_TRY(mvs_conv2d_relu_fwd_packed(buf_a, packed[1], bias[1], buf_b, B, h, wd, 32, 32, stream));
    MVS_TRY(mvs_conv2d_relu_fwd_packed(buf_b, packed[2], bias[2], buf_a, B, h, wd, 32, 32, stream));
    return mvs_refine_tail_eval(buf_a, wtail, btail, depth, out, B, h, wd, stream);
}

// The reverse order.  gout [B,h,w]: gradient of the refined depth.  gbuf[3] / draw[0..2] [B,h,w,32], draw[3] [B,h,w], gx0 [B,h,w,4]:
// work buffers; slots_b[3]: caller-zeroed backward statistic rows of the 32-channel blocks; tail_rec: 512 doubles of scratch.
// Every weight gradient is computed: layers 1, 2 in one launch on the raw activations (mvs_conv2d_wgrad_batch_xf), the 4 -> 32 and
// 32 -> 1 layers, which that launch has no instantiation for, through mvs_conv2d_wgrad.  gimg [B,3,H,W] or NULL; gdepth [B,h,w] =
// gout (the residual's identity branch) + channel 3 of gx0.
extern "C" int mvs_refine_bwd(int frozen, int B, int H, int W, int h, int wd, const float* const* w, const float* x0, const float* const* raw, const float* y2,
                              const float* const* stats, const float* beta3, double* const* slots_b, const int* nslots, double* tail_rec,
                              const float* gout, float* const* gbuf, float* const* draw, float* gx0, float* dgrad_ws, float* const* gw,
                              float* wgrad_ws, float* const* dgamma, float* const* dbeta, float* gimg, float* gdepth, hipStream_t stream) {
    MVS_REQUIRE(x0 && y2 && beta3 && nslots && tail_rec && gout && gx0 && dgrad_ws && wgrad_ws && gdepth && slots_b && gbuf, MVS_ERR_NULL,
                "mvs_refine_bwd: null pointer argument");
    REFINE_P4("mvs_refine_bwd", w); REFINE_P4("mvs_refine_bwd", raw); REFINE_P4("mvs_refine_bwd", stats); REFINE_P4("mvs_refine_bwd", draw);
    REFINE_P4("mvs_refine_bwd", gw); REFINE_P4("mvs_refine_bwd", dgamma); REFINE_P4("mvs_refine_bwd", dbeta);
    for (int i = 0; i < 3; ++i) MVS_REQUIRE(slots_b[i] && gbuf[i], MVS_ERR_NULL, "mvs_refine_bwd: null work buffer of block %d", i);
    MVS_REQUIRE(B >= 1 && H >= 4 && W >= 4 && h == H / 4 && wd == W / 4, MVS_ERR_SHAPE, "mvs_refine_bwd: a [%d,3,%d,%d] image does not go with a [%d,%d,%d] depth map", B, H, W, B, h, wd);
    const long long V = (long long)B * h * wd;
    MVS_TRY(mvs_refine_tail_bwd(gout, raw[3], stats[3], beta3, frozen, V, tail_rec, draw[3], dgamma[3], dbeta[3], stream));
    MVS_TRY(mvs_conv2d_dgrad_wl(draw[3], w[3], gbuf[2], dgrad_ws, B, h, wd, 32, 1, 3, 1, 0, stream));
    for (int i = 2; i >= 0; --i) {
        if (frozen) {
            MVS_TRY(mvs_bn_relu_bwd_frozen(gbuf[i], raw[i], stats[i], slots_b[i], nslots[i], 0, 1, V, 32, draw[i], dgamma[i], dbeta[i], stream));
        } else {
            MVS_TRY(mvs_bn_bwd_reduce_slots(gbuf[i], raw[i], stats[i], 1, 1, V, 32, slots_b[i], nslots[i], stream));
            MVS_TRY(mvs_bn_relu_bwd_slots(gbuf[i], raw[i], stats[i], slots_b[i], nslots[i], 1, 1, V, 32, draw[i], dgamma[i], dbeta[i], stream));
        }
        MVS_TRY(mvs_conv2d_dgrad_wl(draw[i], w[i], i > 0 ? gbuf[i - 1] : gx0, dgrad_ws, B, h, wd, REFINE_CIN[i], 32, 3, 1, 0, stream));
    }
    const float* xs[2] = {raw[0], raw[1]};
    const float* xst[2] = {stats[0], stats[1]};
    const float* gys[2] = {draw[1], draw[2]};
    float* gws[2] = {gw[1], gw[2]};
    const int shapes[16] = {B, h, wd, 32, 32, 3, 1, 0, B, h, wd, 32, 32, 3, 1, 0};
    MVS_TRY(mvs_conv2d_wgrad_batch_xf(2, xs, xst, B, gys, gws, wgrad_ws, shapes, stream));
    MVS_TRY(mvs_conv2d_wgrad(x0, draw[0], gw[0], wgrad_ws, B, h, wd, 4, 32, 3, 1, stream));
    MVS_TRY(mvs_conv2d_wgrad(y2, draw[3], gw[3], wgrad_ws, B, h, wd, 32, 1, 3, 1, stream));
    return mvs_refine_assemble_bwd(gx0, gout, gimg, gdepth, B, H, W, h, wd, stream);
}

// ---- FeaturePyramid of CVP-MVSNet (jdacs-ms/models/network.py:16-50) in training, one C call per pass --------------------------------
// Nine conv 3x3 + bias + LeakyReLU blocks (3 -> 64 -> 64 -> 64 -> 32 -> 32 -> 32 -> 16 -> 16 -> 16), the same weights on S levels of a
// half-size image pyramid; all views are one batch of N images.  Kernels: csrc/pyramid_kernels.h and the igemm family of csrc/conv2d.hip.
// One stream, no allocation, no host synchronisation, no events.  `ws`: mvs_pyramid_workspace_floats(N, H, W, S) floats, laid out by
// pyr_plan below (the forward pass uses only the forward weight images; a pass may be given a fresh buffer).
extern "C" {
int mvs_pyramid_images(const float* img, float* const* out, int N, int H, int W, int S, hipStream_t stream);
int mvs_pyramid_record_rows(int N, int H, int W);
int mvs_pyramid_head_mask(const float* gout, const float* y, float* g, float* rec, int N, int H, int W, int C, float slope, hipStream_t stream);
int mvs_pyramid_grad_finish(int nlayers, const int* cin, const int* cout, const int* w_channels_last, int nlevels, const float* const* slots,
                            const float* const* rec, const int* rows, float* const* gw, float* const* gb, hipStream_t stream);
int mvs_conv2d_lrelu_fwd_packed(const float* x, float* packed, const float* bias, float* y, int N, int H, int W, int Cin, int Cout,
                                float negative_slope, hipStream_t stream);
int mvs_conv2d_pack_dgrad_weights_batch(int n, const float* const* w, float* const* ws, const int* shapes, const int* w_channels_last,
                                        hipStream_t stream);
int mvs_conv2d_dgrad_lrelu_mask(const float* gy, const float* w, const float* y_front, float* gx, float* rec, float* ws, int N, int H, int W,
                                int Cin, int Cout, float slope, int w_channels_last, int ws_packed, hipStream_t stream);
long long mvs_conv2d_workspace_floats(int op, int N, int H, int W, int Cin, int Cout, int ks, int stride);
}

#define MVS_PYR_LAYERS 9
#define MVS_PYR_MAX_LEVELS 6
static const int PYR_CIN[MVS_PYR_LAYERS] = {3, 64, 64, 64, 32, 32, 32, 16, 16}, PYR_COUT[MVS_PYR_LAYERS] = {64, 64, 64, 32, 32, 32, 16, 16, 16};

struct PyrPlan {                      // offsets in floats into `ws`
    int h[MVS_PYR_MAX_LEVELS], w[MVS_PYR_MAX_LEVELS], rows[MVS_PYR_MAX_LEVELS];
    long long fpk[MVS_PYR_LAYERS];    // forward weight images
    long long dpk[MVS_PYR_LAYERS];    // input-gradient weight images of layers 1 .. 8
    long long buf[2];                 // ping-pong gradient buffers [N,H,W,64] of the largest level
    long long slot[MVS_PYR_MAX_LEVELS][MVS_PYR_LAYERS];   // weight-gradient image of (level, layer)
    long long rec[MVS_PYR_MAX_LEVELS][MVS_PYR_LAYERS];    // bias-gradient records [rows][Cout] of (level, layer)
    long long wgws;                   // partial images of one mvs_conv2d_wgrad
    long long total;
};

// the chain (channel counts connect, every layer served by the kernels it will meet) and the levels, before the first launch
static int pyr_plan(const char* what, int S, int N, int H, int W, PyrPlan& p) {
    MVS_REQUIRE(S >= 1 && S <= MVS_PYR_MAX_LEVELS, MVS_ERR_SHAPE, "%s: 1..%d pyramid levels, got %d", what, MVS_PYR_MAX_LEVELS, S);
    MVS_REQUIRE(N >= 1 && H >= 1 && W >= 1 && (long long)N * H * W * 64 < (1LL << 31), MVS_ERR_SHAPE, "%s: bad image batch [%d,3,%d,%d]", what, N, H, W);
    long long off = 0;
    auto take = [&](long long n) { const long long o = off; off += (n + 63) / 64 * 64; return o; };
    long long wg = 0;
    for (int i = 0; i < MVS_PYR_LAYERS; ++i) {
        MVS_REQUIRE(i == 0 || PYR_CIN[i] == PYR_COUT[i - 1], MVS_ERR_SHAPE, "%s: layer %d does not read layer %d's output", what, i, i - 1);
        const long long f = mvs_conv2d_workspace_floats(0, N, H, W, PYR_CIN[i], PYR_COUT[i], 3, 1);
        const long long d = i > 0 ? mvs_conv2d_workspace_floats(1, N, H, W, PYR_CIN[i], PYR_COUT[i], 3, 1) : 0;
        const long long g = mvs_conv2d_workspace_floats(2, N, H, W, PYR_CIN[i], PYR_COUT[i], 3, 1);
        MVS_REQUIRE(f > 0 && d >= 0 && g > 0 && (i == 0 || (PYR_CIN[i] >= 9 && PYR_COUT[i] >= 9)), MVS_ERR_UNSUPPORTED,
                    "%s: layer %d (%d -> %d channels) is not served", what, i, PYR_CIN[i], PYR_COUT[i]);
        p.fpk[i] = take(f);
        p.dpk[i] = take(d);
        if (g > wg) wg = g;
    }
    p.buf[0] = take((long long)N * H * W * 64);
    p.buf[1] = take((long long)N * H * W * 64);
    int h = H, w = W;
    for (int s = 0; s < S; ++s) {
        MVS_REQUIRE(h >= 1 && w >= 1, MVS_ERR_SHAPE, "%s: level %d of a %dx%d image has no pixels (%dx%d)", what, s, H, W, h, w);
        p.h[s] = h; p.w[s] = w; p.rows[s] = mvs_pyramid_record_rows(N, h, w);
        for (int i = 0; i < MVS_PYR_LAYERS; ++i) {
            p.slot[s][i] = take((long long)PYR_COUT[i] * PYR_CIN[i] * 9);
            p.rec[s][i] = take((long long)p.rows[s] * PYR_COUT[i]);
        }
        h /= 2; w /= 2;
    }
    p.wgws = take(wg);
    p.total = off;
    return MVS_OK;
}

extern "C" long long mvs_pyramid_workspace_floats(int N, int H, int W, int S) {
    PyrPlan p;
    return pyr_plan("mvs_pyramid_workspace_floats", S, N, H, W, p) == MVS_OK ? p.total : -1;
}

static int pyr_ptrs(const char* what, const void* const* p, int n, const char* name) {
    MVS_REQUIRE(p, MVS_ERR_NULL, "%s: null pointer argument (%s)", what, name);
    for (int i = 0; i < n; ++i) MVS_REQUIRE(p[i], MVS_ERR_NULL, "%s: %s[%d] is null", what, name, i);
    return MVS_OK;
}
#define PYR_PN(what, p, n) MVS_TRY(pyr_ptrs(what, (const void* const*)(p), n, #p))

// img [N,3,H,W] contiguous -> imgs[s] [N,h_s,w_s,3] (the level images, kept by the caller for the backward pass) and act[s * 9 + i]
// [N,h_s,w_s,Cout_i] (block i's output on level s; act[s * 9 + 8] is the level's feature map).  w[i] [Cout][Cin][3][3], or
// channels-last in memory where w_channels_last[i]; bias[i] [Cout].  Launches: pyramid_images, ONE pack launch for the nine forward
// weight images, 9 S convolutions.
extern "C" int mvs_pyramid_fwd(int S, int N, int H, int W, const float* img, const float* const* w, const float* const* bias,
                               const int* w_channels_last, float slope, float* const* imgs, float* const* act, float* ws, hipStream_t stream) {
    PyrPlan p;
    MVS_TRY(pyr_plan("mvs_pyramid_fwd", S, N, H, W, p));
    MVS_REQUIRE(img && w_channels_last && ws, MVS_ERR_NULL, "mvs_pyramid_fwd: null pointer argument");
    MVS_REQUIRE(slope > 0.f, MVS_ERR_SHAPE, "mvs_pyramid_fwd: the backward pass reads the activation's mask from the outputs, which needs a positive slope, got %g", (double)slope);
    PYR_PN("mvs_pyramid_fwd", w, MVS_PYR_LAYERS); PYR_PN("mvs_pyramid_fwd", bias, MVS_PYR_LAYERS);
    PYR_PN("mvs_pyramid_fwd", imgs, S); PYR_PN("mvs_pyramid_fwd", act, S * MVS_PYR_LAYERS);
    MVS_TRY(mvs_pyramid_images(img, imgs, N, H, W, S, stream));
    float* packed[MVS_PYR_LAYERS];
    int shapes[4 * MVS_PYR_LAYERS];
    for (int i = 0; i < MVS_PYR_LAYERS; ++i) {
        packed[i] = ws + p.fpk[i];
        shapes[4 * i] = PYR_CIN[i]; shapes[4 * i + 1] = PYR_COUT[i]; shapes[4 * i + 2] = 3; shapes[4 * i + 3] = 1;
    }
    MVS_TRY(mvs_conv2d_pack_weights_batch(MVS_PYR_LAYERS, w, packed, shapes, w_channels_last, stream));
    for (int s = 0; s < S; ++s)
        for (int i = 0; i < MVS_PYR_LAYERS; ++i)
            MVS_TRY(mvs_conv2d_lrelu_fwd_packed(i == 0 ? imgs[s] : act[s * MVS_PYR_LAYERS + i - 1], packed[i], bias[i], act[s * MVS_PYR_LAYERS + i], N,
                                                p.h[s], p.w[s], PYR_CIN[i], PYR_COUT[i], slope, stream));
    return MVS_OK;
}

// gout[s] [N,h_s,w_s,16] or NULL (a level without a gradient contributes nothing and launches nothing) -> gw[i] (the parameter's
// memory layout) and gb[i] [Cout] of all nine layers; a NULL gw[i] / gb[i] is not computed.  Launches: ONE pack launch for the eight
// input-gradient weight images; per level with a gradient the head (mask of block 8), then from layer 8 down to 1 the layer's weight
// gradient (mvs_conv2d_wgrad into the (level, layer) slot) and its masked input gradient into the other ping-pong buffer, then layer
// 0's weight gradient on the level image; ONE pyramid_grad_finish.
extern "C" int mvs_pyramid_bwd(int S, int N, int H, int W, const float* const* w, const int* w_channels_last, float slope,
                               const float* const* imgs, const float* const* act, const float* const* gout, float* const* gw, float* const* gb,
                               float* ws, hipStream_t stream) {
    PyrPlan p;
    MVS_TRY(pyr_plan("mvs_pyramid_bwd", S, N, H, W, p));
    MVS_REQUIRE(w_channels_last && gout && gw && gb && ws, MVS_ERR_NULL, "mvs_pyramid_bwd: null pointer argument");
    MVS_REQUIRE(slope > 0.f, MVS_ERR_SHAPE, "mvs_pyramid_bwd: the activation's mask is read from the outputs, which needs a positive slope, got %g", (double)slope);
    PYR_PN("mvs_pyramid_bwd", w, MVS_PYR_LAYERS); PYR_PN("mvs_pyramid_bwd", imgs, S); PYR_PN("mvs_pyramid_bwd", act, S * MVS_PYR_LAYERS);
    float* dpk[MVS_PYR_LAYERS - 1];
    int dshapes[2 * (MVS_PYR_LAYERS - 1)];
    for (int i = 1; i < MVS_PYR_LAYERS; ++i) {
        dpk[i - 1] = ws + p.dpk[i];
        dshapes[2 * (i - 1)] = PYR_CIN[i]; dshapes[2 * (i - 1) + 1] = PYR_COUT[i];
    }
    MVS_TRY(mvs_conv2d_pack_dgrad_weights_batch(MVS_PYR_LAYERS - 1, w + 1, dpk, dshapes, w_channels_last + 1, stream));
    const float* slots[MVS_PYR_MAX_LEVELS * MVS_PYR_LAYERS];
    const float* recs[MVS_PYR_MAX_LEVELS * MVS_PYR_LAYERS];
    int rows[MVS_PYR_MAX_LEVELS];
    for (int s = 0; s < S; ++s) {
        rows[s] = p.rows[s];
        const int h = p.h[s], wd = p.w[s];
        const float* const* a = act + s * MVS_PYR_LAYERS;
        for (int i = 0; i < MVS_PYR_LAYERS; ++i) {
            slots[s * MVS_PYR_LAYERS + i] = (gout[s] && gw[i]) ? ws + p.slot[s][i] : nullptr;
            recs[s * MVS_PYR_LAYERS + i] = gout[s] ? ws + p.rec[s][i] : nullptr;
        }
        if (!gout[s]) continue;
        float* cur = ws + p.buf[0];
        float* other = ws + p.buf[1];
        MVS_TRY(mvs_pyramid_head_mask(gout[s], a[MVS_PYR_LAYERS - 1], cur, ws + p.rec[s][MVS_PYR_LAYERS - 1], N, h, wd, PYR_COUT[MVS_PYR_LAYERS - 1], slope,
                                      stream));
        for (int i = MVS_PYR_LAYERS - 1; i >= 1; --i) {
            if (gw[i]) MVS_TRY(mvs_conv2d_wgrad(a[i - 1], cur, ws + p.slot[s][i], ws + p.wgws, N, h, wd, PYR_CIN[i], PYR_COUT[i], 3, 1, stream));
            MVS_TRY(mvs_conv2d_dgrad_lrelu_mask(cur, nullptr, a[i - 1], other, ws + p.rec[s][i - 1], dpk[i - 1], N, h, wd, PYR_CIN[i], PYR_COUT[i], slope, 0, 1,
                                                stream));
            float* t = cur; cur = other; other = t;
        }
        if (gw[0]) MVS_TRY(mvs_conv2d_wgrad(imgs[s], cur, ws + p.slot[s][0], ws + p.wgws, N, h, wd, PYR_CIN[0], PYR_COUT[0], 3, 1, stream));
    }
    return mvs_pyramid_grad_finish(MVS_PYR_LAYERS, PYR_CIN, PYR_COUT, w_channels_last, S, slots, recs, rows, gw, gb, stream);
}
