// The training feature pyramid of CVP-MVSNet (jdacs-ms/models/network.py:16-50) as one autograd node: the kernels around the nine
// 3x3 convolutions, which csrc/conv2d.hip serves (forward: conv + bias + LeakyReLU from a packed image; backward: the input gradient
// with the LeakyReLU mask of the block in front in its epilogue, conv2d_igemm_kernel<.., LM>; weight gradients: mvs_conv2d_wgrad).
//
//   levels[0] = trunk(img); img = F.interpolate(img, scale_factor=0.5, mode='bilinear').detach(); levels[s] = trunk(img)   (network.py:46-50)
//
// pyramid_images_kernel: every level of the image pyramid, channels-last, in ONE launch.  scale_factor = 0.5 without align_corners
// samples level s-1 at 2 * dst + 0.5: weights (0.5, 0.5) on rows 2y, 2y+1 and columns 2x, 2x+1, and h_s = floor(h_{s-1} / 2), so a
// level-s pixel is a function of the aligned 2^s x 2^s block of the input image alone.  The value is the fixed association
// 0.5 * (0.5 * a + 0.5 * b) + 0.5 * (0.5 * c + 0.5 * d) (a, b: the upper row's pair, c, d: the lower row's), iterated level by level over
// the block's quadtree: the result does not depend on which launch computed the level below.  The images carry no gradient.
// pyramid_head_mask_kernel: g = gout * (y > 0 ? 1 : slope) for the LAST block of a level (its output is the level's feature map), and
// the workgroup's per-channel sums of g -> rec [workgroup][C] (plain stores, every row written).
// pyramid_grad_finish_kernel: ONE launch for all layers -- gw[i] = sum over levels (fixed order, fp64, rounded once) of the level's
// weight-gradient image, written in the parameter's memory layout; gb[i] = fp64 sum of all of layer i's records over workgroups and
// levels in a fixed order, rounded once.  No atomics anywhere: two passes give the same bits.
// Included at the END of conv2d.hip (after refine_kernels.h).

#define MVS_PYRAMID_MAX_LEVELS 6
#define MVS_PYRAMID_MAX_LAYERS 9

struct PyrImagesArgs {
    const float* img;                        // [N,3,H,W]
    float* out[MVS_PYRAMID_MAX_LEVELS];      // [N,h_s,w_s,3]
    int h[MVS_PYRAMID_MAX_LEVELS], w[MVS_PYRAMID_MAX_LEVELS];
    long long start[MVS_PYRAMID_MAX_LEVELS + 1];   // first pixel index of level s in the launch's flat pixel range
    int N, H, W, S;
};

// one channel of the level-s pixel whose 2^s x 2^s block starts at p (row stride W): the block's leaves in Z order, partial results
// of every quadtree level in registers (st[l][0..2]: the first three children of the open node of level l)
__device__ __forceinline__ float pyramid_block_value(const float* __restrict__ p, int W, int s) {
    float st[MVS_PYRAMID_MAX_LEVELS - 1][3];
    float v = 0.f;
    const int leaves = 1 << (2 * s);
#pragma unroll 1
    for (int i = 0; i < leaves; ++i) {
        int yo = 0, xo = 0;
#pragma unroll
        for (int l = 0; l < MVS_PYRAMID_MAX_LEVELS - 1; ++l) {
            xo |= ((i >> (2 * l)) & 1) << l;
            yo |= ((i >> (2 * l + 1)) & 1) << l;
        }
        v = p[(size_t)yo * W + xo];
        bool open = true;
#pragma unroll
        for (int l = 0; l < MVS_PYRAMID_MAX_LEVELS - 1; ++l) {
            if (open && l < s) {
                const int k = (i >> (2 * l)) & 3;          // which child of its level-(l+1) node this finished level-l value is
                if (k == 3) v = 0.5f * (0.5f * st[l][0] + 0.5f * st[l][1]) + 0.5f * (0.5f * st[l][2] + 0.5f * v);
                else {
                    if (k == 0) st[l][0] = v;
                    else if (k == 1) st[l][1] = v;
                    else st[l][2] = v;
                    open = false;
                }
            }
        }
    }
    return v;
}

__global__ __launch_bounds__(256) void pyramid_images_kernel(PyrImagesArgs a) {
    const size_t cs = (size_t)a.H * a.W;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.start[a.S]; i += (long long)gridDim.x * 256) {
        int s = 0;
        while (s + 1 < a.S && i >= a.start[s + 1]) ++s;
        const long long j = i - a.start[s];
        const int x = (int)(j % a.w[s]);
        const long long t = j / a.w[s];
        const int y = (int)(t % a.h[s]), n = (int)(t / a.h[s]);
        const float* __restrict__ p = a.img + (size_t)n * 3 * cs + ((size_t)y << s) * a.W + ((size_t)x << s);   // rows (y << s) + 2^s - 1 < H
        float* __restrict__ o = a.out[s] + 3 * j;
        o[0] = pyramid_block_value(p, a.W, s);
        o[1] = pyramid_block_value(p + cs, a.W, s);
        o[2] = pyramid_block_value(p + 2 * cs, a.W, s);
    }
}

// n4 float4 groups of gout / y / g [rows of C channels]; C in {4, 8, 16, 32, 64}, so a thread meets the same channel quad in every
// round of the grid-stride loop (256 % (C / 4) == 0)
__global__ __launch_bounds__(256) void pyramid_head_mask_kernel(const float* __restrict__ gout, const float* __restrict__ y,
                                                                float* __restrict__ g, float* __restrict__ rec, long long n4, int C,
                                                                float slope) {
    __shared__ float red[256 * 4];
    const int tid = threadIdx.x;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + tid; i < n4; i += (long long)gridDim.x * 256) {
        const float4 gv = *reinterpret_cast<const float4*>(gout + 4 * i), yv = *reinterpret_cast<const float4*>(y + 4 * i);
        float4 o;
        o.x = yv.x > 0.f ? gv.x : gv.x * slope; o.y = yv.y > 0.f ? gv.y : gv.y * slope;
        o.z = yv.z > 0.f ? gv.z : gv.z * slope; o.w = yv.w > 0.f ? gv.w : gv.w * slope;
        *reinterpret_cast<float4*>(g + 4 * i) = o;
        s0 += o.x; s1 += o.y; s2 += o.z; s3 += o.w;
    }
    red[4 * tid] = s0; red[4 * tid + 1] = s1; red[4 * tid + 2] = s2; red[4 * tid + 3] = s3;
    __syncthreads();
    if (tid < C) {        // channel tid: element tid & 3 of the threads whose quad is tid >> 2, in thread order
        const int cq = C / 4;
        double t = 0.0;
        for (int k = tid >> 2; k < 256; k += cq) t += (double)red[4 * k + (tid & 3)];
        rec[(size_t)blockIdx.x * C + tid] = (float)t;
    }
}

struct PyrFinishArgs {
    const float* slot[MVS_PYRAMID_MAX_LEVELS][MVS_PYRAMID_MAX_LAYERS];   // [Cout][Cin][3][3] weight-gradient image of (level, layer), or null
    const float* rec[MVS_PYRAMID_MAX_LEVELS][MVS_PYRAMID_MAX_LAYERS];    // [rows[level]][Cout] records of (level, layer), or null
    int rows[MVS_PYRAMID_MAX_LEVELS];
    float* gw[MVS_PYRAMID_MAX_LAYERS];
    float* gb[MVS_PYRAMID_MAX_LAYERS];
    int cin[MVS_PYRAMID_MAX_LAYERS], cout[MVS_PYRAMID_MAX_LAYERS], wcl[MVS_PYRAMID_MAX_LAYERS];
    int blk0[2 * MVS_PYRAMID_MAX_LAYERS + 1];     // first workgroup of job j: jobs 0 .. n-1 the weights, n .. 2n-1 the biases
    int nlayers, nlevels;
};

__global__ __launch_bounds__(256) void pyramid_grad_finish_kernel(PyrFinishArgs a) {
    __shared__ double red[64 * 16];
    int job = 0;
    while (job + 1 < 2 * a.nlayers && (int)blockIdx.x >= a.blk0[job + 1]) ++job;
    const int b = blockIdx.x - a.blk0[job], tid = threadIdx.x;
    if (job < a.nlayers) {            // 256 elements of layer `job`'s weight gradient
        const int i = job, cin = a.cin[i], n = a.cout[i] * cin * 9, e = b * 256 + tid;
        if (e >= n) return;
        double t = 0.0;
        for (int s = 0; s < a.nlevels; ++s)
            if (a.slot[s][i]) t += (double)a.slot[s][i][e];
        const int tap = e % 9, ci = (e / 9) % cin, co = e / (9 * cin);
        a.gw[i][a.wcl[i] ? ((size_t)co * 9 + tap) * cin + ci : (size_t)e] = (float)t;
        return;
    }
    // 16 channels of layer i's bias gradient: thread = (row slice 0..63, channel quad 0..3); slices meet in LDS in a fixed order
    const int i = job - a.nlayers, C = a.cout[i], c0 = 16 * b + 4 * (tid & 3), slice = tid >> 2;
    double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
    for (int s = 0; s < a.nlevels; ++s) {
        const float* __restrict__ r = a.rec[s][i];
        if (!r || c0 >= C) continue;
        for (int row = slice; row < a.rows[s]; row += 64) {
            const float* __restrict__ q = r + (size_t)row * C + c0;
            if (c0 + 3 < C && (C & 3) == 0) {
                const float4 v = *reinterpret_cast<const float4*>(q);
                t0 += (double)v.x; t1 += (double)v.y; t2 += (double)v.z; t3 += (double)v.w;
            } else {
                t0 += (double)q[0];
                if (c0 + 1 < C) t1 += (double)q[1];
                if (c0 + 2 < C) t2 += (double)q[2];
                if (c0 + 3 < C) t3 += (double)q[3];
            }
        }
    }
    double* d = red + slice * 16 + 4 * (tid & 3);
    d[0] = t0; d[1] = t1; d[2] = t2; d[3] = t3;
    __syncthreads();
    if (tid < 16 && 16 * b + tid < C) {
        double t = 0.0;
        for (int k = 0; k < 64; ++k) t += red[k * 16 + tid];
        a.gb[i][16 * b + tid] = (float)t;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
// img [N,3,H,W] contiguous fp32 -> out[s] [N,h_s,w_s,3], s = 0 .. S-1 (h_0 = H, h_s = floor(h_{s-1} / 2)); a level with a side below
// one pixel is refused
extern "C" int mvs_pyramid_images(const float* img, float* const* out, int N, int H, int W, int S, hipStream_t stream) {
    MVS_REQUIRE(img && out, MVS_ERR_NULL, "pyramid_images: null pointer argument");
    MVS_REQUIRE(S >= 1 && S <= MVS_PYRAMID_MAX_LEVELS, MVS_ERR_SHAPE, "pyramid_images: 1..%d levels, got %d", MVS_PYRAMID_MAX_LEVELS, S);
    MVS_REQUIRE(N >= 1 && H >= 1 && W >= 1 && (long long)N * 3 * H * W < (1LL << 40), MVS_ERR_SHAPE, "pyramid_images: bad image shape [%d,3,%d,%d]", N, H, W);
    PyrImagesArgs a = {};
    a.img = img; a.N = N; a.H = H; a.W = W; a.S = S;
    int h = H, w = W;
    for (int s = 0; s < S; ++s) {
        MVS_REQUIRE(h >= 1 && w >= 1, MVS_ERR_SHAPE, "pyramid_images: level %d of a %dx%d image has no pixels (%dx%d)", s, H, W, h, w);
        MVS_REQUIRE(out[s], MVS_ERR_NULL, "pyramid_images: out[%d] is null", s);
        a.out[s] = out[s]; a.h[s] = h; a.w[s] = w;
        a.start[s + 1] = a.start[s] + (long long)N * h * w;
        h /= 2; w /= 2;
    }
    MVS_LAUNCH(pyramid_images_kernel, dim3(refine_grid(a.start[S], 4096)), dim3(256), 0, stream, a);
    return mvs_check_launch("pyramid_images");
}

// gout / y / g [N,H,W,C] channels-last (16-byte aligned), C in {4, 8, 16, 32, 64}; rec [mvs_pyramid_record_rows(N,H,W)][C]
extern "C" int mvs_pyramid_head_mask(const float* gout, const float* y, float* g, float* rec, int N, int H, int W, int C, float slope,
                                     hipStream_t stream) {
    MVS_REQUIRE(gout && y && g && rec, MVS_ERR_NULL, "pyramid_head_mask: null pointer argument");
    const int rows = mvs_pyramid_record_rows(N, H, W);
    MVS_REQUIRE(rows > 0, MVS_ERR_SHAPE, "pyramid_head_mask: bad shape N=%d H=%d W=%d", N, H, W);
    MVS_REQUIRE(C == 4 || C == 8 || C == 16 || C == 32 || C == 64, MVS_ERR_UNSUPPORTED, "pyramid_head_mask: 4, 8, 16, 32 or 64 channels, got %d", C);
    MVS_REQUIRE(slope > 0.f, MVS_ERR_SHAPE, "pyramid_head_mask: the mask is read from the block's output, which needs a positive slope, got %g", (double)slope);
    MVS_REQUIRE(refine_al16(gout) && refine_al16(y) && refine_al16(g), MVS_ERR_UNSUPPORTED, "pyramid_head_mask: the tensors must be 16-byte aligned");
    MVS_LAUNCH(pyramid_head_mask_kernel, dim3(rows), dim3(256), 0, stream, gout, y, g, rec, (long long)N * H * W * (C / 4), C, slope);
    return mvs_check_launch("pyramid_head_mask");
}

// slots / rec: [nlevels][nlayers] tables (row-major; a null entry contributes nothing), rows[nlevels]: record rows of each level;
// gw[i] (layout of the parameter: [Cout][Cin][3][3], or [Cout][3][3][Cin] when w_channels_last[i]) / gb[i] [Cout]; a null gw[i] or
// gb[i] is not computed
extern "C" int mvs_pyramid_grad_finish(int nlayers, const int* cin, const int* cout, const int* w_channels_last, int nlevels,
                                       const float* const* slots, const float* const* rec, const int* rows, float* const* gw, float* const* gb,
                                       hipStream_t stream) {
    MVS_REQUIRE(cin && cout && w_channels_last && gw && gb && (nlevels == 0 || (slots && rec && rows)), MVS_ERR_NULL, "pyramid_grad_finish: null pointer argument");
    MVS_REQUIRE(nlayers >= 1 && nlayers <= MVS_PYRAMID_MAX_LAYERS && nlevels >= 0 && nlevels <= MVS_PYRAMID_MAX_LEVELS, MVS_ERR_SHAPE,
                "pyramid_grad_finish: 1..%d layers and 0..%d levels, got %d and %d", MVS_PYRAMID_MAX_LAYERS, MVS_PYRAMID_MAX_LEVELS, nlayers, nlevels);
    PyrFinishArgs a = {};
    a.nlayers = nlayers; a.nlevels = nlevels;
    for (int s = 0; s < nlevels; ++s) {
        MVS_REQUIRE(rows[s] >= 1, MVS_ERR_SHAPE, "pyramid_grad_finish: level %d has %d record rows", s, rows[s]);
        a.rows[s] = rows[s];
        for (int i = 0; i < nlayers; ++i) { a.slot[s][i] = slots[s * nlayers + i]; a.rec[s][i] = rec[s * nlayers + i]; }
    }
    int blk = 0;
    for (int i = 0; i < nlayers; ++i) {
        MVS_REQUIRE(cin[i] >= 1 && cin[i] <= 64 && cout[i] >= 1 && cout[i] <= 64, MVS_ERR_UNSUPPORTED, "pyramid_grad_finish: layer %d has %d -> %d channels (1..64)", i, cin[i], cout[i]);
        a.cin[i] = cin[i]; a.cout[i] = cout[i]; a.wcl[i] = w_channels_last[i] ? 1 : 0; a.gw[i] = gw[i]; a.gb[i] = gb[i];
        a.blk0[i] = blk;
        blk += gw[i] ? mvs_cdiv(cout[i] * cin[i] * 9, 256) : 0;
    }
    for (int i = 0; i < nlayers; ++i) {
        a.blk0[nlayers + i] = blk;
        blk += gb[i] ? mvs_cdiv(cout[i], 16) : 0;
    }
    a.blk0[2 * nlayers] = blk;
    if (blk > 0) MVS_LAUNCH(pyramid_grad_finish_kernel, dim3(blk), dim3(256), 0, stream, a);
    return mvs_check_launch("pyramid_grad_finish");
}
