/* mvs_hip.h -- C ABI of libmvs_hip.so: the MI355X (gfx950) hot path of Self-Supervised-MVS.
 *
 * The reference (ToughStoneX/Self-Supervised-MVS) has NO native boundary on this path: the path is
 * a sequence of ATen calls inside two nn.Module.forward()s.  Each entry point below therefore cites
 * the reference Python it replaces (paths relative to the reference root); INTEGRATION.md shows the
 * ctypes stub a maintainer would add on the reference side.
 *
 * Conventions
 *  - All pointers are DEVICE pointers owned by the caller (e.g. PyTorch's caching allocator); the
 *    library never allocates, frees or retains them.  Outputs are fully overwritten unless stated.
 *  - Work is enqueued on `stream` only; no call synchronises the device.  Re-entrant: the last-error
 *    string and the launch trace are thread local.  The one piece of process-wide mutable state is
 *    the tuning knobs (mvs_set_tuning): the launchers read them unsynchronised, so change them only
 *    while no other thread is inside the library.
 *  - fp32 everywhere.  Feature maps are channels-last [B,H,W,C]; volumes channels-last [B,D,H,W,C]
 *    (== torch.channels_last / torch.channels_last_3d memory formats of NCHW / NCDHW tensors).
 *  - Return value: 0 on success, negative on error (MVS_ERR_*), message via mvs_last_error().
 */
#ifndef MVS_HIP_H
#define MVS_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP_PLATFORM_AMD__
typedef struct ihipStream_t* hipStream_t; /* same opaque type as <hip/hip_runtime_api.h> */
#endif

#define MVS_OK 0
#define MVS_ERR_SHAPE (-1)
#define MVS_ERR_UNSUPPORTED (-2)
#define MVS_ERR_LAUNCH (-3)
#define MVS_ERR_NULL (-4)
#define MVS_MAX_SRC 10

int mvs_version(void);              /* 100 == 0.1.0 */
const char* mvs_last_error(void);   /* thread-local, valid until the next failing call */
int mvs_is_emulation(void);         /* 0 in the product library */
/* Launch trace (tests, diagnosis): every kernel launch the library checks notes a label naming the kernel and, where one label
 * would cover several size-selected instantiations, which one ("conv_pers nw=8", "conv_igemm s1_small", "conv_wgrad_reduce wide").
 * Writes the labels of this thread's launches since the previous call, comma-joined, into buf (cap bytes with the terminator;
 * whole labels only; the first 64 are kept) and forgets them.  Returns the number of launches since the previous call.
 * buf == NULL only clears.  Thread local, no allocation, no device work. */
int mvs_launch_trace(char* buf, int cap);
/* Measurement knobs: integers that choose between kernels where the library has more than one (A/B runs, tests of the
 * size-selected variants).  Full-string keys; an unknown key is MVS_ERR_UNSUPPORTED; a value outside the knob's range is clamped.
 * The authoritative list with ranges, defaults and meanings is csrc/tuning.h ("bwd_cpt" is accepted and ignored); some defaults
 * are mirrored in _lib.DEFAULT_TUNING and checked by tests/test_capi_symbols.py.  Process-wide (see Conventions). */
int mvs_set_tuning(const char* key, int value);
int mvs_get_tuning(const char* key, int* value);   /* the knob's current value (a freshly loaded library: its default) */

/* ---- K1/K2: homography warp + variance cost volume -------------------------------------------
 * Replaces homo_warping + the sum / sum-of-squares / variance chain:
 *   jdacs/models/module.py:105-140 (homo_warping), jdacs/models/mvsnet.py:120-136 (variance);
 *   jdacs-ms/models/modules.py:62-104 (homo_warping), :209-261 (proj_cost, per-pixel hypotheses),
 *   jdacs-ms/models/network.py:114-137 (coarse variance, in-place alias quirk => ms_alias=1).
 * ref, srcs[i]: [B,H,W,C] (N-1 source pointers, HOST array of device pointers); rot [B,N-1,9] and
 * trans [B,N-1,3] are rot=proj[:3,:3], trans=proj[:3,3] of src_proj @ inverse(ref_proj)
 * (module.py:116-118), computed by the caller.  depth: [B,D] or, if depth_is_per_pixel, [B,D,H,W].
 * align_corners: 0 = what F.grid_sample does on torch>=1.3 for the reference's call (default),
 * 1 = torch 1.1 behaviour.  C in {8,16,32}.  var_out: [B,D,H,W,C]. */
int mvs_plane_sweep_variance_fwd(const float* ref, const float* const* srcs, const float* rot, const float* trans,
                                 const float* depth, int depth_is_per_pixel, int B, int N, int C, int D, int H,
                                 int W, int align_corners, int ms_alias, float* var_out, hipStream_t stream);
/* The same volume stored in bf16 ([B,D,H,W,C], round to nearest even): the inference path of BASELINE configs[4] (MVSNet
 * N=7, 1600x1184, D=256: 1.94 GB instead of 3.9 GB).  C in {16,32}; 1, 2, 3, 4 or 6 source views.  The reference has no
 * reduced-precision path; this replaces the same lines as mvs_plane_sweep_variance_fwd. */
int mvs_plane_sweep_variance_fwd_bf16(const float* ref, const float* const* srcs, const float* rot, const float* trans,
                                      const float* depth, int depth_is_per_pixel, int B, int N, int C, int D, int H,
                                      int W, int align_corners, int ms_alias, void* var_out_bf16, hipStream_t stream);
/* rot [B,NS,9] / trans [B,NS,3] of src_proj[b,s] @ inverse(ref_proj[b]) for all NS source views in ONE launch (the caller-side
 * lines jdacs/models/module.py:116-118, jdacs-ms/models/modules.py:71-80 run once per view).  src_proj [B,NS,4,4], ref_proj
 * [B,4,4], row-major fp32; fp64 inside.  A singular ref_proj yields inf / nan (like torch.linalg.inv_ex), not an error. */
int mvs_relative_projection(const float* src_proj, const float* ref_proj, int B, int NS, float* rot, float* trans,
                            hipStream_t stream);
/* Backward of the above w.r.t. the feature maps (the reference builds the sampling grid under
 * no_grad, module.py:115).  grad_ref and grad_srcs[i] ([B,H,W,C]) must be ZERO-FILLED by the caller
 * (accumulated with atomics). */
int mvs_plane_sweep_variance_bwd(const float* grad_var, const float* ref, const float* const* srcs,
                                 const float* rot, const float* trans, const float* depth, int depth_is_per_pixel,
                                 int B, int N, int C, int D, int H, int W, int align_corners, int ms_alias,
                                 float* grad_ref, float* const* grad_srcs, hipStream_t stream);

/* homo_warping alone (jdacs/models/module.py:105-140): warped volume [B,D,H,W,C] of ONE source view
 * and its backward (grad_src zero-filled by the caller). */
int mvs_homo_warp_fwd(const float* src, const float* rot, const float* trans, const float* depth,
                      int depth_is_per_pixel, int B, int C, int D, int H, int W, int align_corners,
                      float* warped_out, hipStream_t stream);
int mvs_homo_warp_bwd(const float* grad_warped, const float* src, const float* rot, const float* trans,
                      const float* depth, int depth_is_per_pixel, int B, int C, int D, int H, int W,
                      int align_corners, float* grad_src, hipStream_t stream);

/* ---- K3-K8: 3-D convolutions of CostRegNet ------------------------------------------------------
 * Replace nn.Conv3d / nn.ConvTranspose3d (k=3, pad=1, bias=False; stride 1|2; transposed stride 2
 * has output_padding 1, stride 1 has 0) forward / input-gradient / weight-gradient:
 *   jdacs/models/module.py:35-42, jdacs/models/mvsnet.py:40-63; jdacs-ms/models/network.py:47-65.
 * (D,H,W) are ALWAYS the spatial dims of the forward op's input x.  Weights are the PyTorch
 * parameter tensors as they are: conv [Cout][Cin][3][3][3], transposed conv [Cin][Cout][3][3][3].
 * ws: workspace of mvs_conv3d_workspace_bytes(op,...) bytes, 16-byte aligned.
 * Forward epilogue (any subset): scale&&shift -> y*scale[c]+shift[c] (folded eval BatchNorm);
 * shift only -> y+shift[c] (bias of the prob layer, mvsnet.py:63); relu; + skip (added AFTER the
 * ReLU, mvsnet.py:70-72); stat_slots != NULL -> per-channel (sum, sum of squares) of the RAW conv output are
 * added (fp64 atomics) into row (workgroup mod nslots) of stat_slots [nslots][2][Cout] for train-mode BatchNorm
 * (module.py:39); the caller zeroes the rows, nslots is a power of two (mvs_bn_slots(Cout)); consumer: mvs_bn_relu_fwd_slots.
 * ws_packed = 1: ws already holds this op's weight image (mvs_conv3d_pack_weights[_batch] for the same op and shape). */
enum { MVS_OP_CONV_FWD = 0, MVS_OP_CONV_DGRAD = 1, MVS_OP_CONV_WGRAD = 2,
       MVS_OP_CONVT_FWD = 3, MVS_OP_CONVT_DGRAD = 4, MVS_OP_CONVT_WGRAD = 5 };
long long mvs_conv3d_workspace_bytes(int op, int B, int D, int H, int W, int Cin, int Cout, int stride);
/* Write the MFMA-fragment weight image of a forward / input-gradient op into ws ahead of time -- one launch for one op, or ONE
 * launch for a whole list (ops[n], w[n], ws[n], shapes[n][7] = B, D, H, W, Cin, Cout, stride): the regulariser packs all of its
 * layers once per training step instead of once in front of every convolution. */
int mvs_conv3d_pack_weights(int op, const float* w, float* ws, int B, int D, int H, int W, int Cin, int Cout, int stride,
                            hipStream_t stream);
int mvs_conv3d_pack_weights_batch(int n, const int* ops, const float* const* w, float* const* ws, const int* shapes,
                                  hipStream_t stream);
int mvs_conv3d_fwd(const float* x, const float* w, float* y, float* ws, int B, int D, int H, int W, int Cin, int Cout,
                   int stride, const float* scale, const float* shift, const float* skip, int relu,
                   double* stat_slots, int nslots, int ws_packed, hipStream_t stream);
/* Input gradients: gx = d conv / dx (+ add: [B,D,H,W,Cin] like gx, or NULL).  A tensor with two consumers -- the U-Net skip
 * connections, jdacs/models/mvsnet.py:70-72, jdacs-ms/models/network.py:71-72 -- receives its second gradient contribution in the
 * epilogue of the kernel that computes the first, instead of autograd's separate add pass over both.
 * bn_raw != NULL (like gx): x came out of a BatchNorm+ReLU block, x = relu(BatchNorm(bn_raw)) (+ skip), and gx is that block's
 * COMPLETE output gradient: the epilogue also adds the block's backward statistics (sum dyh, sum dyh*xhat per channel; dyh = gx where
 * the ReLU was active) into bn_slots [nslots][2][Cin] (fp64), from bn_stats [4][Cin] = mean, invstd, scale, shift of the block
 * (backward of module.py:35-42) -- no separate reduction pass over (gx, bn_raw); consumer: mvs_bn_relu_bwd_slots. */
int mvs_conv3d_dgrad(const float* gy, const float* w, const float* add, float* gx, float* ws, int B, int D, int H, int W, int Cin,
                     int Cout, int stride, const float* bn_raw, const float* bn_stats, double* bn_slots, int nslots, int ws_packed,
                     hipStream_t stream);
int mvs_conv3d_wgrad(const float* x, const float* gy, float* gw, float* ws, int B, int D, int H, int W, int Cin,
                     int Cout, int stride, hipStream_t stream);
int mvs_convT3d_fwd(const float* x, const float* w, float* y, float* ws, int B, int D, int H, int W, int Cin,
                    int Cout, int stride, const float* scale, const float* shift, const float* skip, int relu,
                    double* stat_slots, int nslots, int ws_packed, hipStream_t stream);
int mvs_convT3d_dgrad(const float* gy, const float* w, const float* add, float* gx, float* ws, int B, int D, int H, int W, int Cin,
                      int Cout, int stride, const float* bn_raw, const float* bn_stats, double* bn_slots, int nslots, int ws_packed,
                      hipStream_t stream);
int mvs_convT3d_wgrad(const float* x, const float* gy, float* gw, float* ws, int B, int D, int H, int W, int Cin,
                      int Cout, int stride, hipStream_t stream);

/* ---- One call per PASS of a cost-volume regulariser ------------------------------------------------------------------
 * Replace the whole of CostRegNet.forward (jdacs/models/mvsnet.py:66-74, jdacs-ms/models/network.py:67-74) in train mode and
 * its autograd backward: the same kernels as the per-layer entry points above, in the same order, enqueued from C (the
 * per-layer calls cost the launch thread ~1.7 ms per training step from Python).  Nothing is allocated: the caller supplies
 * every tensor (channels-last-3d fp32; sizes follow from the block table).
 * Block i: input = output of block src (-1: x), conv / transposed conv (k3 p1, bias-free; mvs_conv3d_fwd conventions, weight
 * image packed[i] already written by mvs_conv3d_pack_weights_batch) -> BatchNorm(train, statistic slots slots[i] zeroed by the
 * caller, running statistics updated) -> ReLU, + output of block skip (-1: none) AFTER the ReLU (mvsnet.py:70-72).
 * (cin, cout, d, h, w): channels and the spatial dims of the block's INPUT.  The closing prob layer (mvsnet.py:63): stride-1
 * convolution of block n-1's output with bias bprob, prob_cout output channels, workspace ws_prob (mvs_conv3d_workspace_bytes).
 * mvs_unet_fwd outputs: raw[i] (pre-BatchNorm), y[i] (block output), stats[i] [4][cout] (mean, invstd, scale, shift), logits.
 * mvs_unet_bwd: glogits -> gx (or NULL), gw[n+1] (weight gradients in the parameters' layouts; entry n = prob; a NULL entry
 *   is skipped), dgamma[i], dbeta[i]; work space: gbuf[i], draw[i] (each like y[i]), wgrad_ws[n+1] (mvs_conv3d_workspace_bytes
 *   of the WGRAD ops), slots_b[i] (zeroed backward statistic slots), packed_dgrad[n+1] (input-gradient weight images; entry i
 *   may be NULL when block i reads x and gx is NULL).  side_stream != NULL and != main_stream: every weight gradient is
 *   enqueued there behind a HIP event recorded on main_stream after the block's input gradient; join != 0: main_stream waits
 *   for side_stream at the end; *side_stream_used (may be NULL) reports whether anything went to side_stream.
 *   MVS_ERR_UNSUPPORTED for a program that needs an explicit gradient add (a block with two consumers through their INPUT, or
 *   a skip contribution that is not the first): neither reference network is one. */
#define MVS_UNET_MAX_BLOCKS 32
typedef struct MvsUnetBlock {
    int transposed, stride, src, skip;
    float eps, momentum;
    int cin, cout, d, h, w;
} MvsUnetBlock;
int mvs_unet_fwd(int n, const MvsUnetBlock* blocks, int B, const float* x, const float* const* w, const float* const* gamma,
                 const float* const* beta, float* const* running_mean, float* const* running_var, float* const* packed,
                 float* const* raw, float* const* y, float* const* stats, double* const* slots, const int* nslots,
                 const float* wprob, const float* bprob, int prob_cout, float* ws_prob, float* logits, hipStream_t stream);
int mvs_unet_bwd(int n, const MvsUnetBlock* blocks, int B, const float* x, const float* const* w, const float* wprob, int prob_cout,
                 const float* const* y, const float* const* raw, const float* const* stats, double* const* slots_b, const int* nslots,
                 float* const* packed_dgrad, const float* glogits, float* const* gbuf, float* const* draw, float* gx,
                 float* const* gw, float* const* wgrad_ws, float* const* dgamma, float* const* dbeta, hipStream_t main_stream,
                 hipStream_t side_stream, int join, int* side_stream_used);

/* Measurement hook of mvs_unet_bwd (process-wide, like mvs_set_tuning): HIP events around the weight gradient of ONE block
 * (0..n-1, n = the prob layer; < 0: off) on the stream it runs on; mvs_unet_time_read waits for them, writes the durations in
 * ms (launch order, at most max_n) and returns how many there were. */
int mvs_unet_time_wgrad(int block);
int mvs_unet_time_read(float* ms, int max_n);

/* ---- bf16-storage inference path of CostRegNet (BASELINE configs[4]) ------------------------------------------------
 * The same layers (jdacs/models/mvsnet.py:40-63) evaluated as in jdacs/eval.py:143 (eval mode, no_grad) with activations
 * stored in bf16 and fp32 accumulation (v_mfma_f32_16x16x32_bf16).  x, skip: bf16 [B,D,H,W,C]; w: the fp32 parameter;
 * y: bf16, or fp32 when out_is_f32 (the probability layer's logits).  transposed: stride 2 only.  Epilogue as
 * mvs_conv3d_fwd without statistics.  Supported (Cin -> Cout): the network's layer shapes -- stride 1: 32->8, 8->8, 16->8,
 * 16->16, 32->32, 64->64, 8->1, 16->1; stride 2: 8->16, 16->32, 32->64; transposed: 64->32, 32->16, 16->8.
 * ws: mvs_conv3d_bf16_workspace_bytes(...) bytes (packed bf16 weight image), 16-byte aligned. */
long long mvs_conv3d_bf16_workspace_bytes(int Cin, int Cout, int stride, int transposed);
int mvs_conv3d_bf16_fwd(const void* x_bf16, const float* w, void* y, void* ws, int B, int D, int H, int W, int Cin, int Cout,
                        int stride, int transposed, const float* scale, const float* shift, const void* skip_bf16, int relu,
                        int out_is_f32, hipStream_t stream);
int mvs_cast_f32_bf16(const float* x, void* y_bf16, long long n, hipStream_t stream);   /* n % 4 == 0 */

/* ---- BatchNorm3d / BatchNorm2d (+ReLU, + post-ReLU skip add) on channels-last [V][C] -----------
 * Replace nn.BatchNorm3d + F.relu of ConvBnReLU3D (module.py:35-42) and of the deconv blocks (mvsnet.py:48-61), and
 * nn.BatchNorm2d + F.relu of the 2-D ConvBnReLU (module.py:15-22).  C in {4,8,16,32,64}.
 * Train mode works on "statistic slots": nslots rows [2][C] of fp64 accumulators per statistics group, zeroed by the caller,
 * into which the PRODUCER of the tensor adds per-workgroup sums -- a convolution epilogue (mvs_conv3d_fwd / mvs_convT3d_fwd /
 * mvs_conv2d_fwd_stats; backward: mvs_conv3d_dgrad / mvs_convT3d_dgrad with bn_raw) or the stand-alone passes below -- and which
 * the APPLY kernel finishes in the prologue of every workgroup (no finalize launch in between).
 * G statistics groups of Vg contiguous rows each share the affine parameters; the running statistics are updated group after
 * group == G successive BatchNorm calls: the N views of a sample go through the shared-weight feature extractor as one batch
 * (jdacs/models/mvsnet.py:115) with the reference's per-view statistics.  slots [G][nslots][2][C]; stats [G][4][C] = mean, invstd
 * (biased variance, eps), scale = gamma*invstd, shift = beta - mean*scale (written by the forward, read by the backward). */
int mvs_bn_slots(int C);   /* recommended nslots (power of two; 16 KB of accumulators per group) */
int mvs_bn_stats_slots(const float* x, int G, long long Vg, int C, double* slots, int nslots, hipStream_t stream);
/* y = relu?(BatchNorm_train(x)) (+ skip); running_mean / running_var (both or neither NULL) updated with `momentum` and the
 * unbiased variance (PyTorch defaults) */
int mvs_bn_relu_fwd_slots(const float* x, const double* slots, int nslots, int G, long long Vg, int C, const float* gamma,
                          const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                          const float* skip, int relu, float* stats, float* y, hipStream_t stream);
/* backward statistics (sum dyh, sum dyh*xhat) of dy = grad w.r.t. relu?(bn(x)) into slots, when no input-gradient epilogue did */
int mvs_bn_bwd_reduce_slots(const float* dy, const float* x, const float* stats, int relu, int G, long long Vg, int C,
                            double* slots, int nslots, hipStream_t stream);
/* dx [G*Vg][C] = BatchNorm+ReLU backward of dy given the slots; dgamma [C], dbeta [C] (summed over the groups; may be NULL) */
int mvs_bn_relu_bwd_slots(const float* dy, const float* x, const float* stats, const double* slots, int nslots, int relu, int G,
                          long long Vg, int C, float* dx, float* dgamma, float* dbeta, hipStream_t stream);
int mvs_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                       float eps, int C, float* scale, float* shift, hipStream_t stream);
/* y = relu?(x*scale+shift) (+ skip) */
int mvs_bn_relu_fwd(const float* x, const float* scale, const float* shift, const float* skip, int relu, long long V,
                    int C, float* y, hipStream_t stream);
/* Frozen statistics with a gradient: nn.BatchNorm2d / nn.BatchNorm3d in .eval() inside a model that trains (module.py:15-22,35-42
 * under model.train() + bn.eval(), or model.eval() with autograd on).  stats [4][C] = running_mean, invstd = 1/sqrt(running_var +
 * eps), scale = gamma/sqrt(running_var + eps), shift = beta - running_mean*scale: the layout of the train-mode stats, so the
 * bn_raw epilogues of mvs_conv3d_dgrad / mvs_convT3d_dgrad take it as it is.  Forward: mvs_bn_relu_fwd with rows 2 and 3. */
int mvs_bn_frozen_stats(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                        int C, float* stats, hipStream_t stream);
/* draw [V][C] = scale * dyh, dyh = dy * [raw*scale + shift > 0] (relu); dbeta = sum dyh, dgamma = sum dyh * (raw - running_mean) *
 * invstd through fp64 slot rows [nslots][2][C].  dgamma == dbeta == NULL: one launch, no reduction, slots unused.  have_sums != 0:
 * the slots already hold the two sums (an input-gradient epilogue was given `stats`): one launch.  have_sums == 0: caller-zeroed
 * rows, filled by the pass and finished by a one-workgroup launch.  The running statistics are never written. */
int mvs_bn_relu_bwd_frozen(const float* dy, const float* raw, const float* stats, double* slots, int nslots, int have_sums,
                           int relu, long long V, int C, float* draw, float* dgamma, float* dbeta, hipStream_t stream);

/* ---- mvsnet_loss (jdacs/models/mvsnet.py:164-166): mean smooth-L1 (beta 1) of est - gt over the n pixels with mask > 0.5 ----
 * forward: out[0] = loss (nan for an empty mask, like the reference's mean over an empty selection), out[1] = pixel count;
 * backward: gest[i] = [mask > 0.5] * clamp(est - gt, -1, 1) * gloss[0] / out[1].  Two launches instead of ~14. */
int mvs_masked_smooth_l1_fwd(const float* est, const float* gt, const float* mask, long long n, float* out, hipStream_t stream);
int mvs_masked_smooth_l1_bwd(const float* est, const float* gt, const float* mask, const float* fwd_out, const float* gloss,
                             long long n, float* gest, hipStream_t stream);

/* ---- the seven depth-map validation metrics of one (est, gt, mask) triple (csrc/depth_metrics_kernels.h) -------------------------
 * Replaces AbsDepthError_metrics and Thres_metrics with their per-image wrapper (jdacs/utils.py:134-163, the same text in
 * jdacs-ms/utils.py) and non_zero_mean_absolute_diff / less_one_percentage / less_three_percentage (jdacs/losses/unsup_loss.py:
 * 86-125, jdacs-ms/losses/unsup_loss.py:89-128) as train.py calls them in a block (jdacs/train.py:232-238, :319-325,
 * jdacs-ms/train.py:271-277), and DictAverageMeter.update (jdacs/utils.py:112-131) for these values.
 * est, gt [B,HW] fp32 (device).  mask [B,HW]: torch.bool bytes (mask_is_byte != 0, non-zero = selected) or fp32 (selected where
 * > 0.5).  interval [B] fp32 (device) or NULL: then mae, less_one and less_three come out NaN.  thresholds: HOST array of T floats,
 * 0 <= T <= 8 (copied into the launch; NULL allowed for T = 0).
 * out [4+T] (device): abs error, the T rates of |est - gt| > threshold (strict), mae, less_one, less_three.  per_image [B,2+T]: abs
 * error and the T rates of every image, then the image's term of mae.  Abs error and rates are means over the image's mask, then
 * the mean over images (an empty mask: NaN); mae is the SUM over images of (sum |[gt != 0] (gt - est)| / interval_b) / (count_b +
 * 1e-7); less_k = sum [gt != 0][|gt - est| / interval_b <= k] / (sum [gt != 0] + 1e-7) over the whole batch.  NaN inputs fall where
 * the reference's comparisons put them.  Counts are exact integers, turned into fp32 once at the division: equal to the reference's
 * fp32 sums of ones below 2^24 pixels per image (per batch for less_k).
 * meter / meter_count (both or neither): fp64 [4+T] running sums to which out is added, and one 64-bit call counter.
 * ws: mvs_depth_metrics_workspace_bytes() bytes = B * ceil(HW / 4096) tile records of 64 bytes; the query answers -1 for B outside
 * 1..65535, HW < 1 or T outside 0..8.  Two launches, no atomics, no host synchronisation; the same bits on every run and for
 * either mask type. */
long long mvs_depth_metrics_workspace_bytes(int B, int HW, int T);
int mvs_depth_metrics(const float* est, const float* gt, const void* mask, int mask_is_byte, const float* interval,
                      const float* thresholds, int T, int B, int HW, void* ws, float* out, float* per_image, double* meter,
                      long long* meter_count, hipStream_t stream);

/* ---- training-sample preparation: the step's image tensors from the decoded 8-bit views (csrc/sample_prep_kernels.h) ------------
 * Replaces, per view, center_image (jdacs/datasets/dtu_yao.py:94-99, jdacs-ms/dataset/dtu.py:112-119), transform_aug + x255 +
 * center_image (dtu_yao.py:59-63, 241-247, 279-281; dtu.py:80-84, 164-166, 207-219), transform_seg (dtu_yao.py:64-67, 237-239;
 * dtu.py:85-86, 160-162), random_image_mask on the reference view with the mask's F.interpolate(scale_factor=0.25) (jdacs/train.py:
 * 269-275), and the transform chain of Augmentor (jdacs/models/augmentations.py:20-104).
 * src (device), M views: src_kind 0 = u8 [M,H,W,3] as decoded, src_kind 1 = fp32 [M,3,H,W] in [0,1], quantised on load as ToPILImage
 * does (x255, truncated).  src_image_stride: elements between two views (0 = 3 H W), so a row-prefix crop needs no copy.
 * params: HOST fp32 [M,9] or NULL (then imgs_aug must be NULL): four operation ids in application order (0 brightness, 1 contrast,
 * 2 saturation, 3 hue, -1 none; each at most once), their four factors, gamma (> 0).  rect: HOST int [M,4] (y, x, fh, fw) or NULL:
 * the window of random_image_mask, fh = 0 for none.  Both are checked and copied into the launches' arguments.
 * Arithmetic, fp32 on values in [0,1]: gray = 0.299 r + 0.587 g + 0.114 b; brightness clamp(f x); contrast clamp(f x + (1 - f)
 * mean_HW(gray of the image as it stands)); saturation clamp(f x + (1 - f) gray); hue through hsv with colorsys's conventions,
 * h = (h + f) mod 1; gamma clamp(x^gamma); all clamps to [0,1].  center_image: per channel (x - mean) / (sqrt(var) + 1e-8) with
 * the population mean and variance over H W, from exact integer sums (imgs) or fp64 sums (imgs_aug), evaluated in fp64 and
 * rounded once.
 * Outputs (device, each may be NULL, not all): imgs = center_image(u8); imgs_aug = the chain, then x255 and center_image when
 * aug_center != 0 (the loaders' form) or left in [0,1] (Augmentor's), then times the window mask; imgs_seg = (u8 / 255 - mean_c) /
 * std_c with the ImageNet constants; all three logically [M,3,H,W], stored as such or as [M,H,W,3] when channels_last != 0.
 * filter_mask [M, H / s, W / s] fp32 for s = mask_scale in {1, 4}: the mask's value at pixel (s i, s j), sizes floored.
 * ws: mvs_sample_prep_workspace_bytes() bytes = M * ceil(H W / 4096) tile records of 128 bytes; the query answers -1 for M, H or
 * W < 1 or M H W 3 >= 2^31.  Three launches per 64 views (two when imgs_aug is absent or not centred), no atomics, no host
 * synchronisation, the same bits on every run.  Bad sizes, a null workspace or a bad operation id return a negative code and
 * launch nothing. */
long long mvs_sample_prep_workspace_bytes(int M, int H, int W);
int mvs_sample_prep(const void* src, int src_kind, long long src_image_stride, const float* params, const int* rect, float* imgs,
                    float* imgs_aug, float* imgs_seg, float* filter_mask, int mask_scale, int aug_center, int channels_last, int M,
                    int H, int W, void* ws, hipStream_t stream);

/* ---- The optimiser step: Adam over the flat parameter store, one launch (csrc/adam_kernels.h) --------------------------------
 * Replaces optim.Adam(model.parameters(), lr, betas=(0.9, 0.999), weight_decay=wd).step() of jdacs/train.py:71,208 and
 * jdacs-ms/train.py:101,260 for parameters that are views of ONE flat fp32 store (dist.FlatGradBucket(flatten_params=True)).
 * For element i, all fp32:  g = grad[i] * grad_scale (+ weight_decay * p[i] when weight_decay != 0: torch's L2 form, not AdamW);
 *   m[i] += (1 - beta1) (g - m[i]);  v[i] = beta2 v[i] + (1 - beta2) g g;  p[i] -= (lr / bc1) m[i] / (sqrt(v[i]) / sqrt(bc2) + eps)
 * with bc = 1 - beta^t; the constants are formed in fp64 and rounded to fp32 once.  grad_scale carries the 1/world of a summed
 * all-reduce.  p, m, v: flat [n] device arrays, updated in place; 16-byte accesses where the actual addresses allow, any alignment
 * and any n work.
 * step_counter: device int[2], owned by the optimiser: [0] = steps taken so far, [1] = scratch that is 0 between calls (zero both
 * to start).  The step t = [0] + 1 is read on the device and [0] is advanced by exactly 1 per call, so a launch captured into a
 * graph stays correct on replay; lr and the other hyper-parameters are arguments and ARE baked into a captured launch.
 * mvs_adam_step: grad flat [n] (the packed bucket).  One launch, trace label "adam_flat".
 * mvs_adam_step_table: the gradient of flat range [offsets[k], offsets[k] + counts[k]) is read from grads[k] (HOST arrays of nseg
 *   entries; grads[k] a device pointer of counts[k] floats with 4-byte alignment, or NULL = a gradient of zeros).  Segments must be
 *   sorted by offset, non-empty, disjoint and inside [0, n); elements that no segment covers are left untouched.  The table travels
 *   in the kernel arguments: one launch ("adam_table") per MVS_ADAM_MAX_SEGMENTS = 128 segments, earlier launches of a longer table
 *   are labelled "adam_table part" and only the last advances the counter.  Bit-identical to mvs_adam_step on the packed gradients.
 * mvs_adam_limits: the workgroup's chunk of flat elements and the segments per launch (for tests of the boundary cases).
 * Checked on the host before any launch: null pointers, n <= 0 (MVS_ERR_SHAPE) or n above 2^31 - 2049 (MVS_ERR_UNSUPPORTED), the
 * segment rules, lr < 0, betas outside [0, 1), eps < 0, weight_decay < 0, non-finite hyper-parameters. */
int mvs_adam_limits(int* chunk, int* max_segments);
int mvs_adam_step(float* p, const float* grad, float* m, float* v, long long n, int* step_counter, double lr, double beta1,
                  double beta2, double eps, double weight_decay, double grad_scale, hipStream_t stream);
int mvs_adam_step_table(float* p, float* m, float* v, long long n, const float* const* grads, const long long* offsets,
                        const long long* counts, int nseg, int* step_counter, double lr, double beta1, double beta2, double eps,
                        double weight_decay, double grad_scale, hipStream_t stream);

/* ---- K9/K10: softmax over depth + soft-argmin regression + photometric confidence --------------
 * Replace F.softmax(dim=1) + depth_regression + the pad/avg_pool3d/gather confidence:
 *   jdacs/models/mvsnet.py:141-151, jdacs/models/module.py:145-148;
 *   jdacs-ms/models/network.py:147-149,173-189, jdacs-ms/models/modules.py:324-331.
 * logits [B,D,H,W]; depth [B,D] or [B,D,H,W]; outputs [B,H,W].  save_max/save_sum (may be NULL in
 * inference) are the per-pixel softmax max and denominator the backward needs. */
int mvs_softargmin_conf_fwd(const float* logits, const float* depth, int depth_is_per_pixel, int B, int D, int H,
                            int W, float* out_depth, float* out_conf, float* save_max, float* save_sum,
                            hipStream_t stream);
int mvs_softargmin_conf_bwd(const float* grad_depth, const float* logits, const float* depth, int depth_is_per_pixel,
                            const float* out_depth, const float* save_max, const float* save_sum, int B, int D, int H,
                            int W, float* grad_logits, hipStream_t stream);

/* ---- the self-supervised loss on the path's output ------------------------------------------------
 * Replaces UnSupLoss.forward and its autograd graph (jdacs/losses/unsup_loss.py:24-83; inverse_warping
 * jdacs/losses/homography.py:186-351; compute_reconstr_loss / SSIM / depth_smoothness jdacs/losses/modules.py:17-90).
 * ref, views[v]: quarter-resolution NHWC images [B,H,W,3] (the caller does F.interpolate(0.25, bilinear) + permute,
 * unsup_loss.py:36-37,53-54); kinv [B,9] = K_ref^-1; proj [B,V,12] = K_ref.[R_rel | t_rel] row major
 * (homography.py:200-236: R_rel = R_v R_ref^T, t_rel = t_v - R_rel t_ref; the REFERENCE intrinsics project, as there);
 * depth [B,H,W]; V = number of source views, 3 <= V <= 10 (the top-3 selection needs three).
 * out[4] (device): total = 12 reconstr + 6 ssim + 0.18 smooth, then the three terms.  ws: caller-owned scratch of
 * mvs_unsup_loss_workspace_floats() floats; the backward reads what the forward left there.  grad_out: device scalar.
 * Only the depth map receives a gradient. */
long long mvs_unsup_loss_workspace_floats(int B, int V, int H, int W);
int mvs_unsup_loss_fwd(const float* ref, const float* const* views, const float* kinv, const float* proj,
                       const float* depth, int B, int V, int H, int W, float smooth_lambda, float* ws, float* out,
                       hipStream_t stream);
int mvs_unsup_loss_bwd(const float* ref, const float* const* views, const float* kinv, const float* proj,
                       const float* depth, int B, int V, int H, int W, float smooth_lambda, float* ws,
                       const float* grad_out, float* grad_depth, hipStream_t stream);

/* ---- JDACS co-segmentation, part 1: non-negative matrix factorisation V ~ W H (csrc/seg_loss_kernels.h) -------------------
 * Replaces NMF / multiplicative_update_step / approximation_error (jdacs/models/seg_dff.py:21-106) as SegDFF.forward calls
 * them (:128): P independent problems (one per batch item) in one call, no host synchronisation.
 * V [P,n,m] fp32, non-negative.  W [P,n,k], H [P,k,m]: the initial factors on entry (the caller draws them: |randn| *
 * sqrt(mean(V) / k), W before H; the kernels draw nothing), the result on exit.  update_h = 0: H stays as given and only W is
 * updated (the reference's path for a caller-supplied H, :72-80).
 * Per iteration, in the reference's order: VH = V H^t, HH = H H^t, WHH = W HH, entries == 0 become 1e-7, W *= VH / WHH; then with
 * the NEW W: WV = W^t V, WWH = (W^t W) H, zeros become 1e-7, H *= WV / WWH.  Stopping rule (:91-102): e0 = |V - W H|_F before the
 * first iteration; after iterations 0, 10, 20, ... e = |V - W H|_F, stop when (e_prev - e) / e0 < tol, else e_prev = e.  tol <= 0
 * disables the test (then only e0 is evaluated).  The decision is taken on the device; launches enqueued after it return at once.
 * status [P,4] (device floats): iterations run, number of non-finite entries of the returned W (exact below 2^24), e0, the last e
 * evaluated.  ws: mvs_nmf_workspace_floats() floats (second W buffer, per-workgroup partial rows, the solve state).
 * Limits: 1 <= P <= 65535, 1 <= k <= 8, n >= k, m >= k, n*m < 2^31, 1 <= max_iter <= 100000; no alignment demand on n or m.  The
 * workspace query answers -1 for a shape the solve rejects.  Deterministic: every cross-workgroup sum is partial rows + a
 * fixed-order finish.  2 launches per iteration + 2 (+ 2 when the reference tests after the last iteration). */
long long mvs_nmf_workspace_floats(int P, int n, int m, int k);
int mvs_nmf_solve(const float* V, float* W, float* H, int P, int n, int m, int k, int update_h, int max_iter, float tol,
                  float* ws, float* status, hipStream_t stream);

/* ---- JDACS co-segmentation, part 2: the segmentation loss (csrc/seg_loss_kernels.h) ------------------------------------------
 * Replaces compute_seg_loss (jdacs/losses/unsup_seg_loss.py:21-34) for every source view of UnSupSegLoss.forward (:62-75),
 * with its inverse_warping (jdacs/losses/homography.py:186-351).  ref_seg [B,H,W,K] and view_segs (HOST array of V device
 * pointers [B,H,W,K]) are the segmentation maps already at the depth map's resolution; kinv [B,9], proj [B,V,12], depth [B,H,W]
 * as for mvs_unsup_loss_fwd.  Per source view: logits = the K bilinearly warped values (sample geometry and validity mask of
 * mvs_unsup_loss_fwd), target = index of the FIRST maximum of ref_seg at the pixel, term = mean over all batch items' pixels with
 * mask > 0.5 of logsumexp(logits) - logits[target].  out [1+V] (device): the sum over the views, then every view's term.  A view
 * without a valid pixel gives 0 / 0 = NaN (and so does the sum), as F.cross_entropy on an empty selection does.
 * Backward: only the depth map receives a gradient, through the sample coordinates, with the reference's clamped-index weights;
 * the maps and the mask carry none (seg_dff.py:142).  ws: mvs_seg_loss_workspace_floats() floats, filled by the forward and read
 * by the backward; grad_out: device scalar (gradient of out[0]).
 * Limits: 1 <= V <= 10 (no top-3 selection here, N = 2 works), 2 <= K <= 8, B >= 1, H, W >= 2, B*H*W*K < 2^31.  The workspace
 * query answers -1 otherwise.  Two launches forward, one backward; deterministic reductions. */
long long mvs_seg_loss_workspace_floats(int B, int V, int H, int W, int K);
int mvs_seg_loss_fwd(const float* ref_seg, const float* const* view_segs, const float* kinv, const float* proj,
                     const float* depth, int B, int V, int H, int W, int K, float* ws, float* out, hipStream_t stream);
int mvs_seg_loss_bwd(const float* ref_seg, const float* const* view_segs, const float* kinv, const float* proj,
                     const float* depth, int B, int V, int H, int W, int K, float* ws, const float* grad_out,
                     float* grad_depth, hipStream_t stream);

/* ---- the same loss with its weights as arguments: jdacs-ms UnSupLoss at full resolution --------------------------------
 * Serves jdacs-ms/losses/unsup_loss.py:18-82, which train.py calls once per pyramid level on the depth map nearest-up-sampled to
 * the image size (jdacs-ms/train.py:222-229): total = w_reconstr reconstr + w_ssim ssim + w_smooth smooth (12 / 6 / 0.05
 * there, smooth_lambda 1).  Layouts as above, but ref, views[v] are the FULL-resolution NHWC images [B,H,W,3] (one permute,
 * no interpolation) and depth [B,H,W] is at image resolution; kinv / proj are built from the full-resolution intrinsics.
 * The top-3 selection runs over the grid (one thread per pixel, per-workgroup partial rows with int32 selection counts, one
 * workgroup finishing them in a fixed order) instead of in a single workgroup.  Same selection rule as mvs_unsup_loss_fwd:
 * strict '<' insertion (ties go to the lower view index), entries >= 1e4 contribute nothing.
 * Limits: 3 <= V <= 10, B >= 1, H >= 3, W >= 3, B*H*W <= 2^29 (32-bit pixel offsets); anything else is rejected before any
 * launch with a negative code and a message naming the limit (the workspace query answers -1).
 * Deterministic: no float atomics; every reduction is fixed-order, so two identical calls give bitwise-identical outputs and
 * gradients.  ws: caller-owned scratch of mvs_unsup_loss_weighted_workspace_floats() floats, filled by the forward and read by
 * the backward (same weights).  After the forward, ws[V*n*4 + (4V+2)*ceil(n/256) + 48 + v] (n = B*H*W) holds the number of
 * pixels that selected view v as int32. */
long long mvs_unsup_loss_weighted_workspace_floats(int B, int V, int H, int W);
int mvs_unsup_loss_weighted_fwd(const float* ref, const float* const* views, const float* kinv, const float* proj,
                                const float* depth, int B, int V, int H, int W, float w_reconstr, float w_ssim,
                                float w_smooth, float smooth_lambda, float* ws, float* out, hipStream_t stream);
int mvs_unsup_loss_weighted_bwd(const float* ref, const float* const* views, const float* kinv, const float* proj,
                                const float* depth, int B, int V, int H, int W, float w_reconstr, float w_ssim,
                                float w_smooth, float smooth_lambda, float* ws, const float* grad_out, float* grad_depth,
                                hipStream_t stream);

/* ---- stage glue of CVP-MVSNet --------------------------------------------------------------------
 * Replaces calDepthHypo (jdacs-ms/models/modules.py:107-206): hypos[b,k] = ref_depths[b] + (k - 4) * interval_b, k = 0..7,
 * interval_b = mean over the pixels of |depth change that moves the projection into source view 0 by one pixel along the
 * epipolar line| (fp64 inside, like the reference).  mats [B,30] fp64: K_ref^-1 (9), K_src (E_src E_ref^-1)[:3,:] (12),
 * (K_ref R_ref)(K_src R_src)^-1 (9), prepared by the caller from the camera matrices.  ws: fp64 scratch. */
long long mvs_depth_hypo_workspace_doubles(int B, int H, int W);
int mvs_depth_hypo(const float* ref_depths, const double* mats, int B, int H, int W, double* ws, float* hypos,
                   hipStream_t stream);

/* ---- the rest of the stage glue of a CVP-MVSNet forward (csrc/cvp_stage_kernels.h) ------------------------------------
 * mvs_cvp_cameras: every camera product of one forward in ONE launch, label "cvp_cameras" (replaces conditionIntrinsics, _ms_proj +
 * mvs_relative_projection per level, the host lines of calDepthHypo with their three LU inverses, calSweepingDepthHypo).  fp32
 * inputs ref_in [B,3,3], src_in [B,S,3,3], ref_ex [B,4,4], src_ex [B,S,4,4], depth_min / depth_max [B] (item 0 is read, like the
 * reference); level_h: HOST array of the L level heights, level 0 the finest.  1 <= S <= 10, 1 <= L <= 6.  Outputs:
 *   in_ms  [B,S+1,L,3,3] fp32  rows 0 and 1 of K divided by img_h / level_h[l], row 2 copied; view 0 = reference
 *   rot    [L,B,S,3,3], trans [L,B,S,3] fp32  of (K_s,l E_s[:3,:] ; 0 0 0 1) (K_ref,l E_ref[:3,:] ; 0 0 0 1)^-1
 *   mats   [L-1,B,30] fp64  for the levels 0 .. L-2, source view 0, in mvs_depth_hypo's layout (may be NULL when L == 1)
 *   planes [B,48] fp32  depth_min[0] + i (depth_max[0] - depth_min[0]) / 47
 * Every product reads the conditioned intrinsics as rounded to fp32 (in_ms), is evaluated in fp64 (Gauss-Jordan with partial
 * pivoting; a singular matrix gives inf / nan, no error) and rounded once.
 * mvs_depth_hypo_up: the transition to the next finer level in two launches, labels "depth_hypo_up_interval" and
 * "depth_hypo_up_write": mvs_depth_hypo on the x2 bilinear up-sampling (F.interpolate(scale_factor=2, align_corners=None)) of
 * depth [B,h,w], evaluated per fine pixel inside both launches.  hypos [B,8,2h,2w]; depth_up [B,2h,2w] is written when not NULL;
 * ws: mvs_depth_hypo_workspace_doubles(B, 2h, 2w) doubles.  No atomics: two calls give the same bits. */
int mvs_cvp_cameras(const float* ref_in, const float* src_in, const float* ref_ex, const float* src_ex, const float* depth_min,
                    const float* depth_max, int B, int S, int L, int img_h, const int* level_h, float* in_ms, float* rot,
                    float* trans, double* mats, float* planes, hipStream_t stream);
int mvs_depth_hypo_up(const float* depth, const double* mats, int B, int h, int w, double* ws, float* hypos, float* depth_up,
                      hipStream_t stream);

/* ---- SURVEY.md 8(f)-3, first cut (not used by default): the feature extractors' 2-D convolutions ---------------------
 * nn.Conv2d of jdacs/models/module.py:15-22 as used by FeatureNet (jdacs/models/mvsnet.py:17-34): 3x3 stride 1 pad 1 and
 * 5x5 stride 2 pad 2, 1..32 channels, channels-last images x [N,H,W,Cin], w [Cout][Cin][ks][ks], y [N,Ho,Wo,Cout].
 * op for the workspace query: 0 forward, 1 input gradient, 2 weight gradient; -1 for a shape the op does not serve.
 * Served: forward and input gradient 1..32 or exactly 64 channels on either side (the stride-2 input gradient: Cin <= 32).
 * mvs_conv2d_wgrad has an instantiation per input-channel slice width (Cin rounded up to a multiple of 4, 32 for Cin = 64):
 *   3x3 stride 1: Cin 1..8, 13..16, 29..32, 64     5x5 stride 2: Cin 5..8, 13..16     (Cout 1..32 or 64 in both)
 * anything else is refused by the query (-1) and by the call (MVS_ERR_UNSUPPORTED) before the first launch.
 * Launch labels (mvs_launch_trace) name the instantiation: "conv2d_igemm k3|k5 cc4|8|16|32 nb1|2[ stats| stats+xf| stats+bst]",
 * "conv2d_igemm (pixel pairs) cc4|8[ ...]", "conv2d_dgrad_s2_one_pass|_classes ccN nbN", "conv2d_dgrad_s2" (direct form),
 * "conv2d_wgrad k3|k5 cxpN nbN" per slice + "conv2d_wgrad_reduce wide|narrow", "conv2d_wgrad_batch[ xf]" +
 * "conv2d_wgrad_batch_reduce", "conv2d_pack_weights_batch". */
long long mvs_conv2d_workspace_floats(int op, int N, int H, int W, int Cin, int Cout, int ks, int stride);
int mvs_conv2d_fwd(const float* x, const float* w, const float* bias, float* y, float* ws, int N, int H, int W, int Cin,
                   int Cout, int ks, int stride, hipStream_t stream);
/* conv2d + bias + LeakyReLU(negative_slope) in one pass: the `conv` block of the CVP feature pyramid
 * (jdacs-ms/models/modules.py:15-19, network.py:16-41; widths 3/16/32/64).  Channels: 1..32 or exactly 64. */
/* conv2d forward (no bias) that also adds BatchNorm's statistics of its output into slots [G][nslots][2][Cout] (fp64, zeroed by
 * the caller): the N images are G statistics groups of N/G consecutive images; consumer: mvs_bn_relu_fwd_slots.
 * The convolution + statistics half of ConvBnReLU in training (jdacs/models/module.py:15-22). */
int mvs_conv2d_fwd_stats(const float* x, const float* w, float* y, float* ws, double* slots, int nslots, int G, int N, int H,
                         int W, int Cin, int Cout, int ks, int stride, int ws_packed, hipStream_t stream);
/* Forward weight images of n layers in ONE launch (then mvs_conv2d_fwd_stats(..., ws_packed = 1) skips its own packing launch):
 * w[n] parameter tensors [Cout][Cin][ks][ks] -- or channels-last in memory ([Cout][ks][ks][Cin]) where w_channels_last[i] --,
 * ws[n] workspaces of mvs_conv2d_workspace_floats(0, ...) floats, shapes[n][4] = Cin, Cout, ks, stride. */
int mvs_conv2d_pack_weights_batch(int n, const float* const* w, float* const* ws, const int* shapes, const int* w_channels_last,
                                  hipStream_t stream);
int mvs_conv2d_lrelu_fwd(const float* x, const float* w, const float* bias, float* y, float* ws, int N, int H, int W, int Cin,
                         int Cout, int ks, int stride, float negative_slope, hipStream_t stream);
int mvs_conv2d_dgrad(const float* gy, const float* w, float* gx, float* ws, int N, int H, int W, int Cin, int Cout, int ks,
                     int stride, hipStream_t stream);
/* mvs_conv2d_fwd with the parameter tensor channels-last in memory ([Cout][ks][ks][Cin]) when w_channels_last: read in place. */
int mvs_conv2d_fwd_wl(const float* x, const float* w, const float* bias, float* y, float* ws, int N, int H, int W, int Cin, int Cout,
                      int ks, int stride, int w_channels_last, hipStream_t stream);
/* mvs_conv2d_dgrad with the parameter tensor channels-last in memory ([Cout][ks][ks][Cin]) when w_channels_last: read in place. */
int mvs_conv2d_dgrad_wl(const float* gy, const float* w, float* gx, float* ws, int N, int H, int W, int Cin, int Cout, int ks,
                        int stride, int w_channels_last, hipStream_t stream);
int mvs_conv2d_wgrad(const float* x, const float* gy, float* gw, float* ws, int N, int H, int W, int Cin, int Cout, int ks,
                     int stride, hipStream_t stream);
/* Weight gradients of up to 8 layers in ONE launch + one reduction launch (the training extractor's backward pass: replaces the
 * weight half of the convolution_backward nodes autograd builds for jdacs/models/module.py:18 `self.conv` of every ConvBnReLU of
 * jdacs/models/mvsnet.py:21-31 and for mvsnet.py:32 `self.feature`).  shapes[n][8] = N, H, W, Cin, Cout, ks, stride,
 * w_channels_last; x[i] [N,H,W,Cin], gy[i] [N,Ho,Wo,Cout] (NHWC, pad ks/2); gw[i] is written as [Cout][Cin][ks][ks], or as
 * [Cout][ks][ks][Cin] when w_channels_last (the memory of a channels_last nn.Conv2d weight).  Served layers: 3x3 stride 1 with
 * 3 / 8 / 16 -> <= 16 or 32 -> <= 32 channels, 5x5 stride 2 with 8 -> <= 16 or 16 -> <= 32, Cout % 4 == 0.
 * mvs_conv2d_wgrad_batch_workspace_floats: size of ws for these shapes, or -1 if a layer is not served. */
long long mvs_conv2d_wgrad_batch_workspace_floats(int n, const int* shapes);
/* Consumer-side BatchNorm of the training extractor (the host path's default since round 4; MVS_FEATURE_FUSED_APPLY=0 restores the
 * apply passes): block i's `F.relu(self.bn(...))`
 * (jdacs/models/module.py:21-22) is applied by block i+1's convolution -- forward and weight gradient -- while it stages its
 * input, so block i has no apply pass and its normalised output exists nowhere in memory.
 * mvs_bn_finalize_slots: the statistic slots of a block -> stats [G][4][C] (mean, invstd, scale, shift) + running statistics
 *   (the prologue of mvs_bn_relu_fwd_slots without its elementwise pass).
 * mvs_conv2d_fwd_stats_xf: mvs_conv2d_fwd_stats with x = the RAW output of the block in front and in_stats = that block's stats.
 * mvs_conv2d_wgrad_batch_xf: mvs_conv2d_wgrad_batch where x[i] is raw when x_stats[i] is not null (groups of imgs_per_group images). */
int mvs_bn_finalize_slots(const double* slots, int nslots, int G, long long Vg, int C, const float* gamma, const float* beta, float eps,
                          float momentum, float* running_mean, float* running_var, float* stats, hipStream_t stream);
int mvs_conv2d_fwd_stats_xf(const float* x, const float* in_stats, const float* w, float* y, float* ws, double* slots, int nslots,
                            int G, int N, int H, int W, int Cin, int Cout, int ks, int stride, int ws_packed, hipStream_t stream);
/* mvs_conv2d_dgrad_bnstats (opt-in, MVS_FEATURE_DGRAD_BNSTATS=1): mvs_conv2d_dgrad of a 3x3 stride-1 layer whose result is the
 * complete output gradient of the BatchNorm + ReLU block in front (raw output bn_raw [N,H,W,Cin], bn_stats [G][4][Cin]); the epilogue
 * adds that block's backward statistics into bn_slots [G][nslots][2][Cin], so mvs_bn_relu_bwd_slots needs no reduce pass. */
int mvs_conv2d_dgrad_bnstats(const float* gy, const float* w, float* gx, float* ws, int N, int H, int W, int Cin, int Cout, int ks,
                             const float* bn_raw, const float* bn_stats, double* bn_slots, int nslots, int G, hipStream_t stream);
int mvs_conv2d_wgrad_batch_xf(int n, const float* const* x, const float* const* x_stats, int imgs_per_group, const float* const* gy,
                              float* const* gw, float* ws, const int* shapes, hipStream_t stream);
int mvs_conv2d_wgrad_batch(int n, const float* const* x, const float* const* gy, float* const* gw, float* ws, const int* shapes,
                           hipStream_t stream);

/* ---- One C call per pass of the TRAINING feature extractor (round 6; csrc/feature_pass.cpp) ------------------------------------
 * FeatureNet (jdacs/models/mvsnet.py:17-34): n ConvBnReLU blocks (module.py:15-22; 3x3 stride 1 or 5x5 stride 2, bias-free) closed by a
 * 3x3 stride-1 convolution with bias (mvsnet.py:32), on N channels-last images that are G statistics groups of N/G consecutive images
 * (the views of a sample: mvsnet.py:115 calls the extractor once per view).  Replaces the 15 module calls of FeatureNet.forward and
 * the ~30 autograd nodes of its backward pass by two calls that enqueue the same kernels in the same order:
 * mvs_feature_fwd: one pack launch for all forward weight images (packed[i]: mvs_conv2d_workspace_floats(0, ...) floats each), then per
 *   block mvs_conv2d_fwd_stats(_xf) -> raw[i] [N,Ho,Wo,cout] + slots[i] (zeroed by the caller, [G][nslots[i]][2][cout] fp64), and
 *   mvs_bn_finalize_slots -> stats[i] [G][4][cout] (block i's BatchNorm + ReLU is applied by block i+1 while it stages its input);
 *   the LAST block gets mvs_bn_relu_fwd_slots -> y_last; then the closing convolution -> out [N,Ho,Wo,close_cout] (ws_close:
 *   mvs_conv2d_workspace_floats(0, ...)).  Running statistics are updated in place, group after group.
 * mvs_feature_bwd: gout -> gx (or NULL), gw[n+1] (every layer's weight gradient, in the parameter's own memory layout; entry n = the
 *   closing convolution), dgamma[i], dbeta[i].  Work space: gbuf[i] (gradient w.r.t. block i's output, like raw[i]), draw[i] (like
 *   raw[i]), slots_b[i] (zeroed), dgrad_ws (the largest mvs_conv2d_workspace_floats(1, ...) of the chain), wgrad_ws_main / _side
 *   (mvs_conv2d_wgrad_batch_workspace_floats of layers [0, early_from) / [early_from, n]).  0 < early_from < n and side_stream !=
 *   main_stream: the weight gradients of layers early_from .. n are enqueued on side_stream as soon as block early_from's raw-output
 *   gradient exists; main_stream waits for side_stream before the call returns (also on an error); *side_stream_used reports it. */
#define MVS_FEAT_MAX_BLOCKS 7
typedef struct MvsFeatBlock {
    int cin, cout, ks, stride;
    float eps, momentum;
    int w_channels_last;
    int h, w;                         /* spatial dims of the block's INPUT */
} MvsFeatBlock;
int mvs_feature_fwd(int n, const MvsFeatBlock* blocks, int N, int G, const float* x, const float* const* w, const float* const* gamma,
                    const float* const* beta, float* const* running_mean, float* const* running_var, float* const* packed,
                    float* const* raw, float* y_last, float* const* stats, double* const* slots, const int* nslots, const float* wclose,
                    const float* bclose, int close_cout, int close_w_channels_last, float* ws_close, float* out, hipStream_t stream);
int mvs_feature_bwd(int n, const MvsFeatBlock* blocks, int N, int G, const float* x, const float* const* w, const float* wclose,
                    int close_cout, int close_w_channels_last, const float* const* raw, const float* y_last, const float* const* stats,
                    double* const* slots_b, const int* nslots, const float* gout, float* const* gbuf, float* const* draw, float* gx,
                    float* dgrad_ws, float* const* gw, float* wgrad_ws_main, float* wgrad_ws_side, float* const* dgamma,
                    float* const* dbeta, int early_from, hipStream_t main_stream, hipStream_t side_stream, int* side_stream_used);

/* ---- RefineNet (jdacs/models/mvsnet.py:77-92) with no library kernel (csrc/refine_kernels.h, csrc/feature_pass.cpp) -------------
 * out = depth + relu(bn(conv(... ConvBnReLU x3 (cat(bilinear(img, 1/4), depth)) ...))): img [B,3,H,W] fp32 NCHW whose batch stride
 * (in floats) is an argument -- MVSNet passes imgs[:, 0] of [B,N,3,H,W] --, depth [B,h,w] contiguous with h = H/4, w = W/4 (floor);
 * any other depth size is refused (MVS_ERR_SHAPE, both shapes in the message).  Launch labels: "refine_assemble",
 * "refine_assemble_bwd", "refine_tail", "refine_tail frozen", "refine_tail eval", "refine_tail_bwd_reduce", "refine_tail_bwd".
 * mvs_refine_assemble: x0 [B,h,w,4] channels-last (16-byte aligned) = (mean of img's pixels (4y+1..4y+2, 4x+1..4x+2) per colour,
 *   depth): bit-identical to F.interpolate(scale_factor=0.25, mode='bilinear') + cat.  One launch.
 * mvs_refine_assemble_bwd: gx0 [B,h,w,4], gy [B,h,w] -> gimg [B,3,H,W] contiguous (0.25 * gx0 on those four pixels, zero elsewhere;
 *   NULL: not computed) and gdepth [B,h,w] = gy + gx0[..., 3].  One launch, no atomics.
 * mvs_refine_tail_fwd: y = depth + relu(gamma * (raw - mean) * invstd + beta) over raw / depth / y [V] with the batch statistics
 *   finished in fp64 from slots [nslots][2] (sum, sum of squares: what mvs_conv2d_fwd_stats adds for Cout = 1; nslots a power of two
 *   <= 256); writes stats [4] = (mean, invstd, scale, shift) and updates running_mean / running_var [1] (both NULL: not tracked)
 *   with `momentum` and the unbiased variance.
 * mvs_refine_tail_fwd_frozen: the same with stats [4] = mvs_bn_frozen_stats(..., C = 1, ...); writes y only.
 * mvs_refine_tail_bwd: gy [V] -> draw [V] (gradient w.r.t. raw), dgamma / dbeta [1] (NULL: not written).  Two launches: per-workgroup
 *   fp64 records (sum dyh, sum dyh * xhat) into rec (512 doubles of scratch), then the apply pass, which sums them in a fixed order:
 *   two calls give the same bits.  frozen != 0: draw = scale * dyh.  The gradient towards depth is gy itself.
 * mvs_refine_tail_eval: y = depth + relu(conv3x3(x, w) + bias), x [B,h,w,32] channels-last, w [1][32][3][3], bias [1] (BatchNorm
 *   folded in by the caller).  One launch.
 * mvs_conv2d_relu_fwd_packed: y = relu(conv3x3 stride 1 (x) + bias) with the forward weight image already in `packed`
 *   (mvs_conv2d_pack_weights_batch): no pack launch.
 * mvs_refine_fwd / _eval_fwd / _bwd take the image's H, W and the depth map's h, w_ (refused unless h = H/4, w_ = W/4).
 * mvs_refine_fwd: the whole forward pass in train mode (frozen = 0: batch statistics, running statistics updated) or with frozen
 *   statistics (frozen != 0: running_* are only read).  w / gamma / beta / running_* / eps / momentum: the four blocks' parameters
 *   (w[i] contiguous [Cout][Cin][3][3], 4 -> 32 -> 32 -> 32 -> 1).  Caller's buffers: x0 [B,h,w,4]; packed[i]
 *   (mvs_conv2d_workspace_floats(0, ...) floats); raw[0..2] / y2 [B,h,w,32], raw[3] [B,h,w]; stats[i] [4][Cout]; slots[i]
 *   [nslots[i]][2][Cout] fp64, zeroed (nslots[3] a power of two <= 256); out [B,h,w].  10 launches (frozen: 12).
 * mvs_refine_eval_fwd: eval mode without a gradient, 5 launches: packed[3] / bias[3] are the weight images and biases of the three
 *   32-channel blocks with BatchNorm folded in, wtail / btail the folded 32 -> 1 layer; buf_a / buf_b [B,h,w,32].
 * mvs_refine_bwd: gout [B,h,w] -> gw[4] (contiguous, every layer), dgamma[i] / dbeta[i], gimg (or NULL), gdepth.  Work space:
 *   gbuf[0..2], draw[0..2] [B,h,w,32], draw[3] [B,h,w], gx0 [B,h,w,4], slots_b[0..2] (zeroed, like slots), tail_rec (512 doubles),
 *   dgrad_ws (the largest mvs_conv2d_workspace_floats(1, ...) of the four layers), wgrad_ws (the largest of
 *   mvs_conv2d_workspace_floats(2, ...) of layers 0 and 3 and mvs_conv2d_wgrad_batch_workspace_floats of layers 1, 2).  One stream. */
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
int mvs_conv2d_relu_fwd_packed(const float* x, float* packed, const float* bias, float* y, int N, int H, int W, int Cin, int Cout,
                               hipStream_t stream);
int mvs_refine_fwd(int frozen, int B, int H, int W, int h, int w_, const float* img, long long img_batch_stride, const float* depth,
                   const float* const* w, const float* const* gamma, const float* const* beta, float* const* running_mean,
                   float* const* running_var, const float* eps, const float* momentum, float* x0, float* const* packed,
                   float* const* raw, float* y2, float* const* stats, double* const* slots, const int* nslots, float* out,
                   hipStream_t stream);
int mvs_refine_eval_fwd(int B, int H, int W, int h, int w_, const float* img, long long img_batch_stride, const float* depth, float* const* packed,
                        const float* const* bias, const float* wtail, const float* btail, float* x0, float* buf_a, float* buf_b,
                        float* out, hipStream_t stream);
int mvs_refine_bwd(int frozen, int B, int H, int W, int h, int w_, const float* const* w, const float* x0, const float* const* raw, const float* y2,
                   const float* const* stats, const float* beta3, double* const* slots_b, const int* nslots, double* tail_rec,
                   const float* gout, float* const* gbuf, float* const* draw, float* gx0, float* dgrad_ws, float* const* gw,
                   float* wgrad_ws, float* const* dgamma, float* const* dbeta, float* gimg, float* gdepth, hipStream_t stream);

/* ---- FeaturePyramid of CVP-MVSNet in training as one autograd node (csrc/pyramid_kernels.h, csrc/conv2d.hip, csrc/feature_pass.cpp)
 * jdacs-ms/models/network.py:16-50: nine conv 3x3 + bias + LeakyReLU blocks (3 -> 64 -> 64 -> 64 -> 32 -> 32 -> 32 -> 16 -> 16 -> 16)
 * with the same weights on S <= 6 levels of a half-size image pyramid, h_0 = H, h_s = floor(h_{s-1} / 2); all views are one batch
 * of N images.  Every tensor is channels-last fp32, 16-byte aligned.  One stream; nothing is allocated, no host synchronisation, no
 * events, no atomics: two passes give the same bits.  Launch labels: "pyramid_images", "conv2d_pack_weights_batch",
 * "conv2d_igemm k3 ccN nbN" (forward), "conv2d_pack_dgrad_weights_batch", "pyramid_head_mask", "conv2d_igemm k3 ccN nbN lrelu-mask"
 * (cc16 / cc32, nb1 / nb2), "conv2d_wgrad k3 cxpN nbN" + "conv2d_wgrad_reduce wide|narrow", "pyramid_grad_finish".
 * mvs_pyramid_images: img [N,3,H,W] contiguous -> out[s] [N,h_s,w_s,3] for s = 0 .. S-1 in ONE launch.  Level 0 is the layout change;
 *   a pixel of level s is the half-size bilinear resize (F.interpolate(scale_factor=0.5), no align_corners) of level s-1, evaluated
 *   as 0.5 * (0.5 * a + 0.5 * b) + 0.5 * (0.5 * c + 0.5 * d) (a, b the upper row's pair, c, d the lower row's) from its 2^s x 2^s
 *   block of img.  A level with a side below one pixel: MVS_ERR_SHAPE.  No backward (the reference detaches the resized levels; a caller that wants
 *   level 0's gradient towards the images takes the per-layer path).
 * mvs_pyramid_record_rows(N, H, W): rows of a level's record buffers = workgroups of the masked input gradient (8 x 32 pixel tiles).
 * mvs_conv2d_lrelu_fwd_packed: mvs_conv2d_lrelu_fwd with the forward weight image already in `packed`
 *   (mvs_conv2d_pack_weights_batch): no pack launch.
 * mvs_conv2d_pack_dgrad_weights_batch: the input-gradient weight images (transposed, flipped) of n <= 16 3x3 stride-1 layers in ONE
 *   launch; shapes[n][2] = the layer's Cin, Cout; ws[i] >= mvs_conv2d_workspace_floats(1, ..., Cin, Cout, 3, 1) floats.
 * mvs_conv2d_dgrad_lrelu_mask: gx [N,H,W,Cin] = mvs_conv2d_dgrad(gy [N,H,W,Cout]) * (y_front > 0 ? 1 : slope) -- the complete output
 *   gradient of the conv + LeakyReLU block in front, whose saved output y_front [N,H,W,Cin] is (slope > 0) -- and
 *   rec [mvs_pyramid_record_rows(N,H,W)][Cin] = per-workgroup channel sums of gx (plain stores, every row written: no zeroing).  More
 *   than 8 channels on both sides (9..32 or 64).  ws_packed: ws holds the image of mvs_conv2d_pack_dgrad_weights_batch; w is not read.
 * mvs_pyramid_head_mask: g = gout * (y > 0 ? 1 : slope) over [N,H,W,C], C in {4, 8, 16, 32, 64}, and rec as above (float4,
 *   grid-stride loop, one workgroup per record row).
 * mvs_pyramid_grad_finish: ONE launch for nlayers <= 9 layers.  slots / rec: [nlevels][nlayers] tables (row-major) of weight-gradient
 *   images [Cout][Cin][3][3] and record buffers [rows[level]][Cout]; a NULL entry contributes nothing.  gw[i] = the sum over levels,
 *   level 0 first, in fp64, rounded once, written in the parameter's memory layout ([Cout][3][3][Cin] when w_channels_last[i]);
 *   gb[i] = the fp64 sum of layer i's records over rows and levels in a fixed order, rounded once.  A NULL gw[i] / gb[i] is skipped.
 * mvs_pyramid_workspace_floats(N, H, W, S): floats of the `ws` of the two passes (forward and input-gradient weight images, two
 *   ping-pong gradient buffers of the largest level, the per-level weight-gradient slots and record buffers, the partial images of
 *   mvs_conv2d_wgrad -- asked for right before the call: it follows the "wgrad2d_groups" knob); -1 where a shape is not served.
 * mvs_pyramid_fwd: imgs[s] [N,h_s,w_s,3] and act[s * 9 + i] [N,h_s,w_s,Cout_i] are the caller's (kept for the backward pass;
 *   act[s * 9 + 8] is level s's feature map).  w[i] / bias[i]: the nine blocks' parameters, w_channels_last[i] as above.  Launches:
 *   pyramid_images, one pack launch, 9 S convolutions.  Uses only the forward weight images of ws.
 * mvs_pyramid_bwd: gout[s] [N,h_s,w_s,16] or NULL (such a level contributes nothing and launches nothing) -> gw[9], gb[9] (a NULL
 *   entry is not computed).  Launches: one pack launch; per level the head, then from layer 8 down to 1 the layer's mvs_conv2d_wgrad
 *   (into its slot of ws) and its masked input gradient into the other ping-pong buffer, then layer 0's weight gradient; one finish.
 * Both check the chain and the levels before the first launch (MVS_ERR_SHAPE / MVS_ERR_UNSUPPORTED / MVS_ERR_NULL with a message). */
int mvs_pyramid_images(const float* img, float* const* out, int N, int H, int W, int S, hipStream_t stream);
int mvs_pyramid_record_rows(int N, int H, int W);
int mvs_conv2d_lrelu_fwd_packed(const float* x, float* packed, const float* bias, float* y, int N, int H, int W, int Cin, int Cout,
                                float negative_slope, hipStream_t stream);
int mvs_conv2d_pack_dgrad_weights_batch(int n, const float* const* w, float* const* ws, const int* shapes, const int* w_channels_last,
                                        hipStream_t stream);
int mvs_conv2d_dgrad_lrelu_mask(const float* gy, const float* w, const float* y_front, float* gx, float* rec, float* ws, int N, int H, int W,
                                int Cin, int Cout, float slope, int w_channels_last, int ws_packed, hipStream_t stream);
int mvs_pyramid_head_mask(const float* gout, const float* y, float* g, float* rec, int N, int H, int W, int C, float slope,
                          hipStream_t stream);
int mvs_pyramid_grad_finish(int nlayers, const int* cin, const int* cout, const int* w_channels_last, int nlevels,
                            const float* const* slots, const float* const* rec, const int* rows, float* const* gw, float* const* gb,
                            hipStream_t stream);
long long mvs_pyramid_workspace_floats(int N, int H, int W, int S);
int mvs_pyramid_fwd(int S, int N, int H, int W, const float* img, const float* const* w, const float* const* bias,
                    const int* w_channels_last, float slope, float* const* imgs, float* const* act, float* ws, hipStream_t stream);
int mvs_pyramid_bwd(int S, int N, int H, int W, const float* const* w, const int* w_channels_last, float slope, const float* const* imgs,
                    const float* const* act, const float* const* gout, float* const* gw, float* const* gb, float* ws, hipStream_t stream);

/* ---- Wide forward 2-D convolutions: the frozen VGG-style trunk in front of the NMF (csrc/conv2d_wide_kernels.h) -----------------
 * 3x3, stride 1, pad 1, fp32, forward only, channels-last images x [N,H,W,Cin] -> y [N,H,W,Cout]; Cin = 3 or 32..512 and
 * Cout = 32..512 in steps of 32 (the existing mvs_conv2d_* family serves 1..32 or exactly 64 channels).  Implicit GEMM on the
 * 16x16x4 fp32 MFMA over flattened positions; which tile / split-K arm ran is in mvs_launch_trace ("conv2d_wide cin3",
 * "conv2d_wide t128x64", "conv2d_wide t64x64", "conv2d_wide splitk=N" + "conv2d_wide reduce", "pool2x2", "resize_cl").  No
 * atomics: two calls give the same bits.  All pointers 16-byte aligned.
 * mvs_conv2d_wide_packed_floats(Cin, Cout): floats of a layer's weight image; mvs_conv2d_wide_pack_weights fills it from the parameter
 *   w [Cout][Cin][3][3] (w_channels_last: [Cout][3][3][Cin] in memory), read in place.  Pack once per weight version.
 * mvs_conv2d_wide_workspace_floats(N, H, W, Cin, Cout): floats of the `ws` of mvs_conv2d_wide_fwd for this layer (the
 *   full-resolution image in front of a pool and the partial images of a split-K launch); -1 outside the served set.
 * mvs_conv2d_wide_fwd: y = [relu](conv(x) + bias), bias may be NULL; pool: followed by a 2x2 stride-2 max pool (floor on odd sizes),
 *   y is then [N,H/2,W/2,Cout].  ws may be NULL when neither a pool nor a split-K launch needs it.
 * mvs_maxpool2x2_cl: x [N,H,W,C] -> y [N,H/2,W/2,C], C a multiple of 4.
 * mvs_resize_bilinear_cl: x [N,C,H,W] (contiguous) -> y [N,oh,ow,C] by the rule of bilinear interpolation with align_corners = False
 *   (source coordinate max(0, (o + 0.5) * in / out - 0.5)): the resize and the layout change in front of the trunk in one pass.
 * mvs_conv_trunk_fwd: n layers as ONE call -- layer i reads x (i = 0) or the previous output and writes buf_a / buf_b in turn, the last
 *   layer writes out [N,h,w,Cout_last]; packed[i] / bias[i] (NULL entries allowed in bias) per layer; buf_a, buf_b: each the largest
 *   output of layers 0 .. n-2; ws: the largest mvs_conv2d_wide_workspace_floats of the chain.  The same kernels in the same order
 *   as n mvs_conv2d_wide_fwd calls; every layer is checked before the first launch.
 *
 * The *_arith entries (csrc/conv2d_wide_bf16_kernels.h) take the ARITHMETIC of the multiplications as an argument -- an argument and
 * not a tuning knob, because the packed weight image depends on it.  fp32 in, fp32 out and fp32 accumulation in every mode:
 *   MVS_ARITH_F32     the entries without the suffix (same kernels, same bits, same trace labels);
 *   MVS_ARITH_BF16    the bf16 MFMA on operands rounded to nearest-even bf16, one product per multiplication.
 * Any other value is MVS_ERR_UNSUPPORTED (1 was the three-term split "bf16x3": measured, not faster than fp32, not shipped --
 * DESIGN.md section 7).  A layer with Cin = 3 runs the fp32 "conv2d_wide cin3" arm (and takes the fp32 image) in every mode.
 * Trace labels of the other layers: "conv2d_wide bf16 pack" / "conv2d_wide bf16 t128x64" / "... t64x64" / "... splitk=N"
 * (+ "conv2d_wide reduce").  The weight image, the workspace and the forward call of one layer
 * must be given the same arith: mvs_conv2d_wide_packed_bytes_arith (BYTES; -1 outside the served set or for an unknown arith),
 * mvs_conv2d_wide_workspace_floats_arith, mvs_conv2d_wide_pack_weights_arith, mvs_conv2d_wide_fwd_arith, mvs_conv_trunk_fwd_arith. */
#define MVS_ARITH_F32 0
#define MVS_ARITH_BF16 2
#define MVS_TRUNK_MAX_LAYERS 32
typedef struct MvsTrunkLayer {
    int cin, cout, relu, pool_after;
} MvsTrunkLayer;
long long mvs_conv2d_wide_workspace_floats(int N, int H, int W, int Cin, int Cout);
long long mvs_conv2d_wide_packed_floats(int Cin, int Cout);
int mvs_conv2d_wide_pack_weights(const float* w, float* ws, int Cin, int Cout, int w_channels_last, hipStream_t stream);
int mvs_conv2d_wide_fwd(const float* x, const float* packed, const float* bias, float* y, float* ws, int N, int H, int W, int Cin,
                        int Cout, int relu, int pool, hipStream_t stream);
int mvs_maxpool2x2_cl(const float* x, float* y, int N, int H, int W, int C, hipStream_t stream);
int mvs_resize_bilinear_cl(const float* x, float* y, int N, int C, int H, int W, int oh, int ow, hipStream_t stream);
int mvs_conv_trunk_fwd(int n, const MvsTrunkLayer* layers, const float* const* packed, const float* const* bias, const float* x,
                       float* buf_a, float* buf_b, float* ws, float* out, int N, int H, int W, hipStream_t stream);
long long mvs_conv2d_wide_packed_bytes_arith(int Cin, int Cout, int arith);
long long mvs_conv2d_wide_workspace_floats_arith(int N, int H, int W, int Cin, int Cout, int arith);
int mvs_conv2d_wide_pack_weights_arith(const float* w, void* ws, int Cin, int Cout, int w_channels_last, int arith, hipStream_t stream);
int mvs_conv2d_wide_fwd_arith(const float* x, const void* packed, const float* bias, float* y, float* ws, int N, int H, int W, int Cin,
                              int Cout, int relu, int pool, int arith, hipStream_t stream);
int mvs_conv_trunk_fwd_arith(int n, const MvsTrunkLayer* layers, const void* const* packed, const float* const* bias, const float* x,
                             float* buf_a, float* buf_b, float* ws, float* out, int N, int H, int W, int arith, hipStream_t stream);

/* ---- geometric-consistency filter on the path's depth maps ---------------------------------------------
 * Replaces reproject_with_depth + check_geometric_consistency (jdacs/eval.py:169-224) for ALL source views of one
 * reference view, and the accumulation of filter_depth (eval.py:372-385): per pixel and source view, project with the
 * reference depth, look the source depth up (cv2.remap INTER_LINEAR semantics: 1/32-pixel fixed point, border 0), project
 * back, test |p' - p| < pix_thresh and |d' - d| / d < rel_thresh (1 and 0.01 in the reference).
 * depth_ref [H,W]; depth_srcs: HOST array of V device pointers [H,W]; mats: DEVICE array of 18 + 42 V doubles =
 * K_ref^-1 [9], K_ref [9], then per view E_src E_ref^-1 (rows 0-2) [12], K_src [9], K_src^-1 [9], E_ref E_src^-1 (rows 0-2)
 * [12], each formed in float32 like numpy does in the reference.  Outputs: count [H,W] int32 (geo_mask_sum), depth_sum
 * [H,W] fp32 (sum of the consistent reprojected depths); optional (NULL to skip) masks [V,H,W] uint8, reproj [V,H,W] fp32
 * (0 where inconsistent), xy_src [V,2,H,W] fp32 (x2d_src, y2d_src). */
int mvs_geo_consistency(const float* depth_ref, const float* const* depth_srcs, const double* mats, int V, int H, int W,
                        float pix_thresh, float rel_thresh, int* count, float* depth_sum, unsigned char* masks, float* reproj,
                        float* xy_src, hipStream_t stream);

/* ---- depth-map fusion (the `fusibile` CUDA program behind jdacs/fusion/depthfusion.py:366-386) ---------
 * Replaces the kernel `fusibile` (jdacs/fusion/fusibile/fusibile.cu:138-277) for ONE reference camera = one launch of the
 * host loop fusibile.cu:416-421: per pixel, back-project with its depth, project into every other view of `subset`,
 * accept the view when the disparities differ by less than depth_thresh and the normals by less than normal_thresh
 * (radians), average the accepted 3-D points / normals / colours, keep the point when at least num_consistent views agree.
 * normals_depths [V,H,W,4] (normal.xyz, depth): the texture of main.cpp:833-843; images [V,H,W,4] colour as float (or NULL);
 * cams [V,32] floats: P (3x4 row-major) [12], M_inv [9], P(:,3) [3], camera centre C [3], 5 unused  (what
 * cameraGeometryUtils.h:353-440 puts into Camera_cu); subset: DEVICE array of n_subset view ids; f = K(0,0).
 * Texture fetches restate CUDA's linear filtering (1.8 fixed-point weights, clamped addressing): csrc/fusibile.hip header.
 * out_points [H,W,12] = coord.xyz 0, normal.xyz 0, colour.xyz 0 -- all zeros where fewer views agree (fully overwritten). */
int mvs_fusibile_fuse(const float* normals_depths, const float* images, const float* cams, const int* subset, int n_subset,
                      int V, int H, int W, int ref_camera, float f, float depth_thresh, float normal_thresh,
                      int num_consistent, int save_texture, float* out_points, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MVS_HIP_H */
