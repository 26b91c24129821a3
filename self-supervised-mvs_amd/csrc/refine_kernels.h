// RefineNet's head and tail (jdacs/models/mvsnet.py:77-92): the kernels around the four 3x3 convolutions, which csrc/conv2d.hip serves.
//
//   small = F.interpolate(img, scale_factor=0.25, mode='bilinear')        \  refine_assemble_kernel: channels-last x0 [B,h,w,4] in one
//   x0    = torch.cat((small, depth.unsqueeze(1)), dim=1)                 /  launch, img read through its batch stride (imgs[:, 0])
//   ... conv1 4->32, conv2 32->32, conv3 32->32 (ConvBnReLU), res: conv 32->1 -> raw r [B,h,w]
//   out   = depth + relu(bn(r))                                              refine_tail_*: BatchNorm2d(1) + ReLU + residual
//
// scale_factor = 0.25 without align_corners samples the source at 4 * dst + 1.5: weights (0.5, 0.5) on rows 4y+1, 4y+2 and columns
// 4x+1, 4x+2 -- the mean of a 2x2 block; 0.25 * (((p11 + p12) + p21) + p22) is bit-identical to ATen's fp32 result.  Its gradient is
// 0.25 * g on those four pixels and zero on the other twelve of the 4x4 cell and on the rows / columns beyond 4h, 4w: every image
// element has exactly one source, so the backward is a gather (no atomics).
//
// The tail works on ONE channel, which the float4 kernels of bn.hip cannot serve (C in {4, 8, 16, 32, 64}).  Forward statistics arrive
// in the fp64 slot rows [nslots][2] the 32 -> 1 convolution's epilogue fills (mvs_conv2d_fwd_stats with Cout = 1); mean and variance are
// finished in fp64, and the normalisation is applied in the centred form gamma * invstd * (r - mean) + beta: with |mean| >> std the
// scale / shift form r * scale + shift cancels hundreds of ulps.  The backward sums (sum dyh, sum dyh * xhat) are per-workgroup fp64
// records [tiles][2] written with plain stores and summed in a fixed order by every workgroup of the apply pass: two runs are bitwise
// equal, no floating-point atomics (the pattern of depth_metrics_kernels.h / sample_prep_kernels.h).
// Included at the END of conv2d.hip: the eval-mode entry for an already packed weight image calls its c2_run_igemm.

#define MVS_REFINE_TAIL_TILES 256   // most workgroups of the backward reduction == rows of its record buffer

__global__ __launch_bounds__(256) void refine_assemble_kernel(const float* __restrict__ img, long long bstride, const float* __restrict__ depth,
                                                              float* __restrict__ x0, int B, int H, int W, int h, int w) {
    const long long total = (long long)B * h * w;
    const size_t cs = (size_t)H * W;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int x = (int)(i % w);
        const long long t = i / w;
        const int y = (int)(t % h), b = (int)(t / h);
        const float* __restrict__ p = img + (long long)b * bstride + (size_t)(4 * y + 1) * W + (4 * x + 1);   // rows 4y+1, 4y+2 < 4h <= H
        float4 o;
        o.x = 0.25f * (((p[0] + p[1]) + p[W]) + p[W + 1]);
        o.y = 0.25f * (((p[cs] + p[cs + 1]) + p[cs + W]) + p[cs + W + 1]);
        o.z = 0.25f * (((p[2 * cs] + p[2 * cs + 1]) + p[2 * cs + W]) + p[2 * cs + W + 1]);
        o.w = depth[i];
        *reinterpret_cast<float4*>(x0 + 4 * i) = o;
    }
}

// gimg [B,3,H,W] (contiguous; may be null: the image needs no gradient) and gdepth [B,h,w] = gy + gx0[..., 3] (the identity branch
// of the residual plus the depth channel of the first block's input gradient)
__global__ __launch_bounds__(256) void refine_assemble_bwd_kernel(const float* __restrict__ gx0, const float* __restrict__ gy,
                                                                  float* __restrict__ gimg, float* __restrict__ gdepth, int B, int H, int W,
                                                                  int h, int w) {
    const long long nd = (long long)B * h * w, ni = gimg ? (long long)B * 3 * H * W : 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < ni + nd; i += (long long)gridDim.x * 256) {
        if (i < ni) {
            const int X = (int)(i % W);
            long long t = i / W;
            const int Y = (int)(t % H);
            t /= H;
            const int c = (int)(t % 3), b = (int)(t / 3);
            const int y = Y >> 2, x = X >> 2;
            const bool in = y < h && x < w && ((Y + 1) & 2) && ((X + 1) & 2);      // rows / columns 1 and 2 of the 4x4 cell
            gimg[i] = in ? 0.25f * gx0[(((size_t)b * h + y) * w + x) * 4 + c] : 0.f;
        } else {
            const long long j = i - ni;
            gdepth[j] = gy[j] + gx0[4 * j + 3];
        }
    }
}

// totals of n <= 256 rows [n][2] of fp64 (statistic slots with C = 1, or the backward records) in a fixed order; all 256 threads call it
__device__ __forceinline__ void refine_row_totals(const double* __restrict__ rows, int n, double* red, double& s1, double& s2) {
    const int tid = threadIdx.x;
    red[tid] = tid < n ? rows[2 * tid] : 0.0;
    red[256 + tid] = tid < n ? rows[2 * tid + 1] : 0.0;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            red[tid] += red[tid + s];
            red[256 + tid] += red[256 + tid + s];
        }
        __syncthreads();
    }
    s1 = red[0];
    s2 = red[256];
}

// out = depth + relu(sc * (r - mu) + be); n4 float4 groups, then the V - 4 * n4 scalar elements (n4 = 0: unaligned pointers)
__device__ __forceinline__ void refine_tail_apply(const float* __restrict__ raw, const float* __restrict__ depth, float* __restrict__ y,
                                                  long long V, long long n4, float mu, float sc, float be) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float4 r = *reinterpret_cast<const float4*>(raw + 4 * i), d = *reinterpret_cast<const float4*>(depth + 4 * i);
        float4 o;
        o.x = d.x + fmaxf((r.x - mu) * sc + be, 0.f);
        o.y = d.y + fmaxf((r.y - mu) * sc + be, 0.f);
        o.z = d.z + fmaxf((r.z - mu) * sc + be, 0.f);
        o.w = d.w + fmaxf((r.w - mu) * sc + be, 0.f);
        *reinterpret_cast<float4*>(y + 4 * i) = o;
    }
    for (long long i = 4 * n4 + (long long)blockIdx.x * 256 + threadIdx.x; i < V; i += (long long)gridDim.x * 256)
        y[i] = depth[i] + fmaxf((raw[i] - mu) * sc + be, 0.f);
}

// train mode: statistics finished from the slot rows in every workgroup's prologue; workgroup 0 writes stats [4] = (mean, invstd,
// scale, shift) for the backward pass and moves the running statistics (momentum, unbiased variance)
__global__ __launch_bounds__(256) void refine_tail_fwd_kernel(const float* __restrict__ raw, const float* __restrict__ depth,
                                                              const double* __restrict__ slots, int nslots, double count,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                              float momentum, float* running_mean, float* running_var,
                                                              float* __restrict__ stats, float* __restrict__ y, long long V, long long n4) {
    __shared__ double red[512];
    double s1, s2;
    refine_row_totals(slots, nslots, red, s1, s2);
    const double mean = s1 / count;
    double var = s2 / count - mean * mean;     // fp64 sums: |mean| = 300 std still leaves 11 digits
    if (var < 0.0) var = 0.0;
    const float invstd = (float)(1.0 / sqrt(var + (double)eps));
    const float mu = (float)mean, sc = gamma[0] * invstd, be = beta[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        stats[0] = mu; stats[1] = invstd; stats[2] = sc; stats[3] = be - mu * sc;
        if (running_mean) {
            const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
            running_mean[0] = (1.0f - momentum) * running_mean[0] + momentum * (float)mean;
            running_var[0] = (1.0f - momentum) * running_var[0] + momentum * (float)unbiased;
        }
    }
    refine_tail_apply(raw, depth, y, V, n4, mu, sc, be);
}

// frozen statistics: stats [4] = (running_mean, invstd, scale, shift) of mvs_bn_frozen_stats with C = 1; nothing is written but y
__global__ __launch_bounds__(256) void refine_tail_fwd_frozen_kernel(const float* __restrict__ raw, const float* __restrict__ depth,
                                                                     const float* __restrict__ stats, const float* __restrict__ beta,
                                                                     float* __restrict__ y, long long V, long long n4) {
    refine_tail_apply(raw, depth, y, V, n4, stats[0], stats[2], beta[0]);
}

// (sum dyh, sum dyh * xhat) of this workgroup's elements -> rec[blockIdx.x][2]; dyh = gy * [sc * (r - mu) + be > 0]
__global__ __launch_bounds__(256) void refine_tail_bwd_reduce_kernel(const float* __restrict__ gy, const float* __restrict__ raw,
                                                                     const float* __restrict__ stats, const float* __restrict__ beta,
                                                                     long long V, double* __restrict__ rec) {
    __shared__ double red[512];
    const int tid = threadIdx.x;
    const float mu = stats[0], is = stats[1], sc = stats[2], be = beta[0];
    double a1 = 0.0, a2 = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + tid; i < V; i += (long long)gridDim.x * 256) {
        const float c = raw[i] - mu;
        const float g = (c * sc + be > 0.f) ? gy[i] : 0.f;
        a1 += (double)g;
        a2 += (double)(g * (c * is));
    }
    red[tid] = a1;
    red[256 + tid] = a2;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            red[tid] += red[tid + s];
            red[256 + tid] += red[256 + tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        rec[2 * blockIdx.x] = red[0];
        rec[2 * blockIdx.x + 1] = red[256];
    }
}

// draw = sc * (dyh - mean(dyh) - xhat * mean(dyh * xhat)) (batch statistics) or sc * dyh (frozen); workgroup 0 writes
// dbeta = sum dyh and dgamma = sum dyh * xhat.  The identity branch of the residual is gy itself (refine_assemble_bwd_kernel adds it).
__global__ __launch_bounds__(256) void refine_tail_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ raw,
                                                              const float* __restrict__ stats, const float* __restrict__ beta,
                                                              const double* __restrict__ rec, int ntiles, int frozen, double inv_count,
                                                              long long V, float* __restrict__ draw, float* dgamma, float* dbeta) {
    __shared__ double red[512];
    double s1, s2;
    refine_row_totals(rec, ntiles, red, s1, s2);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (dbeta) dbeta[0] = (float)s1;
        if (dgamma) dgamma[0] = (float)s2;
    }
    const float m1 = frozen ? 0.f : (float)(s1 * inv_count), m2 = frozen ? 0.f : (float)(s2 * inv_count);
    const float mu = stats[0], is = stats[1], sc = stats[2], be = beta[0];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < V; i += (long long)gridDim.x * 256) {
        const float c = raw[i] - mu;
        const float g = (c * sc + be > 0.f) ? gy[i] : 0.f;
        draw[i] = sc * (g - m1 - (c * is) * m2);
    }
}

// eval mode: y = depth + relu(conv3x3(x, w) + b) with x [B,h,w,32] channels-last and w [1][32][3][3] (BatchNorm folded in): one output
// channel would use 1 of the MFMA's 16 columns, so this is a VALU kernel -- one pixel per thread, taps in a fixed order
__global__ __launch_bounds__(256) void refine_tail_eval_kernel(const float* __restrict__ x, const float* __restrict__ wt,
                                                               const float* __restrict__ bias, const float* __restrict__ depth,
                                                               float* __restrict__ y, int B, int h, int w) {
    __shared__ __attribute__((aligned(16))) float wl[9 * 32];      // [tap][ci]
    for (int t = threadIdx.x; t < 9 * 32; t += 256) wl[t] = wt[(t & 31) * 9 + (t >> 5)];
    __syncthreads();
    const float b0 = bias[0];
    const long long total = (long long)B * h * w;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int px = (int)(i % w);
        const long long t = i / w;
        const int py = (int)(t % h), b = (int)(t / h);
        float acc = 0.f;
#pragma unroll 1          // one row of taps (24 float4 loads) in flight at a time: all nine unrolled took 328 registers
        for (int ty = 0; ty < 3; ++ty) {
            const int iy = py + ty - 1;
            if (iy < 0 || iy >= h) continue;
#pragma unroll
            for (int tx = 0; tx < 3; ++tx) {
                const int ix = px + tx - 1;
                if (ix < 0 || ix >= w) continue;
                const float* __restrict__ xp = x + (((size_t)b * h + iy) * w + ix) * 32;
                const float* wp = wl + (ty * 3 + tx) * 32;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const float4 v = *reinterpret_cast<const float4*>(xp + 4 * q);
                    const float4 k = *reinterpret_cast<const float4*>(wp + 4 * q);
                    acc = fmaf(v.x, k.x, acc); acc = fmaf(v.y, k.y, acc); acc = fmaf(v.z, k.z, acc); acc = fmaf(v.w, k.w, acc);
                }
            }
        }
        y[i] = depth[i] + fmaxf(acc + b0, 0.f);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
static int refine_grid(long long n, int cap) {
    const long long g = (n + 255) / 256;
    return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}
static bool refine_al16(const void* p) { return ((size_t)p & 15) == 0; }
static int refine_shape(const char* what, int B, int H, int W, int h, int w) {
    MVS_REQUIRE(B >= 1 && H >= 4 && W >= 4 && (long long)B * 3 * H * W < (1LL << 40), MVS_ERR_SHAPE, "%s: bad image shape [%d,3,%d,%d]", what, B, H, W);
    MVS_REQUIRE(h == H / 4 && w == W / 4, MVS_ERR_SHAPE, "%s: a [%d,3,%d,%d] image goes with a [%d,%d,%d] depth map, got [%d,%d,%d]", what, B, H,
                W, B, H / 4, W / 4, B, h, w);
    return MVS_OK;
}

extern "C" int mvs_refine_assemble(const float* img, long long img_batch_stride, const float* depth, float* x0, int B, int H, int W, int h,
                                   int w, hipStream_t stream) {
    int rc = refine_shape("refine_assemble", B, H, W, h, w);
    if (rc) return rc;
    MVS_REQUIRE(img && depth && x0, MVS_ERR_NULL, "refine_assemble: null pointer argument");
    MVS_REQUIRE(img_batch_stride >= 3LL * H * W || B == 1, MVS_ERR_SHAPE, "refine_assemble: batch stride %lld below one [3,%d,%d] image",
                img_batch_stride, H, W);
    MVS_REQUIRE(refine_al16(x0), MVS_ERR_UNSUPPORTED, "refine_assemble: the output must be 16-byte aligned");
    MVS_LAUNCH(refine_assemble_kernel, dim3(refine_grid((long long)B * h * w, 2048)), dim3(256), 0, stream, img, img_batch_stride, depth, x0, B,
               H, W, h, w);
    return mvs_check_launch("refine_assemble");
}

extern "C" int mvs_refine_assemble_bwd(const float* gx0, const float* gy, float* gimg, float* gdepth, int B, int H, int W, int h, int w,
                                       hipStream_t stream) {
    int rc = refine_shape("refine_assemble_bwd", B, H, W, h, w);
    if (rc) return rc;
    MVS_REQUIRE(gx0 && gy && gdepth, MVS_ERR_NULL, "refine_assemble_bwd: null pointer argument");
    const long long n = (long long)B * h * w + (gimg ? (long long)B * 3 * H * W : 0);
    MVS_LAUNCH(refine_assemble_bwd_kernel, dim3(refine_grid(n, 4096)), dim3(256), 0, stream, gx0, gy, gimg, gdepth, B, H, W, h, w);
    return mvs_check_launch("refine_assemble_bwd");
}

static bool refine_slots_ok(int n) { return n >= 1 && n <= 256 && (n & (n - 1)) == 0; }

// raw / depth / y [V]; slots [nslots][2] fp64 (sum, sum of squares of raw: mvs_conv2d_fwd_stats with Cout = 1); gamma / beta /
// running_* [1] (running_* may both be null); stats [4] out
extern "C" int mvs_refine_tail_fwd(const float* raw, const float* depth, const double* slots, int nslots, long long V, const float* gamma,
                                   const float* beta, float eps, float momentum, float* running_mean, float* running_var, float* stats,
                                   float* y, hipStream_t stream) {
    MVS_REQUIRE(raw && depth && slots && gamma && beta && stats && y, MVS_ERR_NULL, "refine_tail_fwd: null pointer argument");
    MVS_REQUIRE(V > 0 && refine_slots_ok(nslots), MVS_ERR_SHAPE, "refine_tail_fwd: bad shape V=%lld slots=%d", V, nslots);
    MVS_REQUIRE((running_mean == nullptr) == (running_var == nullptr), MVS_ERR_NULL, "refine_tail_fwd: running_mean and running_var go together");
    const long long n4 = (refine_al16(raw) && refine_al16(depth) && refine_al16(y)) ? V / 4 : 0;
    MVS_LAUNCH(refine_tail_fwd_kernel, dim3(refine_grid(n4 ? n4 : V, 1024)), dim3(256), 0, stream, raw, depth, slots, nslots, (double)V, gamma,
               beta, eps, momentum, running_mean, running_var, stats, y, V, n4);
    return mvs_check_launch("refine_tail");
}

// stats [4]: mvs_bn_frozen_stats(..., C = 1, ...)
extern "C" int mvs_refine_tail_fwd_frozen(const float* raw, const float* depth, const float* stats, const float* beta, long long V, float* y,
                                          hipStream_t stream) {
    MVS_REQUIRE(raw && depth && stats && beta && y, MVS_ERR_NULL, "refine_tail_fwd_frozen: null pointer argument");
    MVS_REQUIRE(V > 0, MVS_ERR_SHAPE, "refine_tail_fwd_frozen: bad shape V=%lld", V);
    const long long n4 = (refine_al16(raw) && refine_al16(depth) && refine_al16(y)) ? V / 4 : 0;
    MVS_LAUNCH(refine_tail_fwd_frozen_kernel, dim3(refine_grid(n4 ? n4 : V, 1024)), dim3(256), 0, stream, raw, depth, stats, beta, y, V, n4);
    return mvs_check_launch("refine_tail frozen");
}

// gy: gradient of out = depth + relu(bn(raw)) [V]; rec: MVS_REFINE_TAIL_TILES x 2 doubles of scratch (written, then read);
// draw [V], dgamma / dbeta [1] (may be null).  The depth branch's gradient is gy unchanged.
extern "C" int mvs_refine_tail_bwd(const float* gy, const float* raw, const float* stats, const float* beta, int frozen, long long V,
                                   double* rec, float* draw, float* dgamma, float* dbeta, hipStream_t stream) {
    MVS_REQUIRE(gy && raw && stats && beta && rec && draw, MVS_ERR_NULL, "refine_tail_bwd: null pointer argument");
    MVS_REQUIRE(V > 0, MVS_ERR_SHAPE, "refine_tail_bwd: bad shape V=%lld", V);
    const int tiles = refine_grid(V, MVS_REFINE_TAIL_TILES);
    MVS_LAUNCH(refine_tail_bwd_reduce_kernel, dim3(tiles), dim3(256), 0, stream, gy, raw, stats, beta, V, rec);
    int rc = mvs_check_launch("refine_tail_bwd_reduce");
    if (rc) return rc;
    MVS_LAUNCH(refine_tail_bwd_kernel, dim3(refine_grid(V, 1024)), dim3(256), 0, stream, gy, raw, stats, beta, (const double*)rec, tiles,
               frozen ? 1 : 0, 1.0 / (double)V, V, draw, dgamma, dbeta);
    return mvs_check_launch("refine_tail_bwd");
}

// x [B,h,w,32] channels-last (16-byte aligned), w [1][32][3][3], bias [1], depth / y [B,h,w]
extern "C" int mvs_refine_tail_eval(const float* x, const float* w, const float* bias, const float* depth, float* y, int B, int h, int w_,
                                    hipStream_t stream) {
    MVS_REQUIRE(x && w && bias && depth && y, MVS_ERR_NULL, "refine_tail_eval: null pointer argument");
    MVS_REQUIRE(B >= 1 && h >= 1 && w_ >= 1, MVS_ERR_SHAPE, "refine_tail_eval: bad shape [%d,%d,%d]", B, h, w_);
    MVS_REQUIRE(refine_al16(x), MVS_ERR_UNSUPPORTED, "refine_tail_eval: the activation must be 16-byte aligned");
    MVS_LAUNCH(refine_tail_eval_kernel, dim3(refine_grid((long long)B * h * w_, 2048)), dim3(256), 0, stream, x, w, bias, depth, y, B, h, w_);
    return mvs_check_launch("refine_tail eval");
}

// 3x3 stride-1 convolution + bias + ReLU whose forward weight image is already in `packed` (mvs_conv2d_pack_weights_batch): the
// eval-mode blocks of a net whose folded weights change only when its parameters do -- no pack launch per call
extern "C" int mvs_conv2d_relu_fwd_packed(const float* x, float* packed, const float* bias, float* y, int N, int H, int W, int Cin, int Cout,
                                          hipStream_t stream) {
    int rc = c2_check("conv2d_relu_fwd_packed", N, H, W, Cin, Cout, 3, 1);
    if (rc) return rc;
    MVS_REQUIRE(x && packed && y, MVS_ERR_NULL, "conv2d_relu_fwd_packed: null pointer argument");
    return c2_run_igemm(x, nullptr, bias, y, packed, N, H, W, Cin, Cout, 3, 1, 0, stream, 1, 0.f, nullptr, 0, 1, 1);
}
