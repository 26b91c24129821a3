// Training-sample preparation: from the decoded 8-bit views of a sample to the three image tensors a self-supervised step consumes.
// Included by loss.hip; not a translation unit of its own.
//
//   imgs      center_image(u8)                                                 jdacs/datasets/dtu_yao.py:94-99, 279
//                                                                              jdacs-ms/dataset/dtu.py:112-119, 203, 213
//   imgs_aug  ColorJitter -> ToTensor -> RandomGamma(clip) -> x255 -> center_image, times the random_image_mask window
//                                                                              dtu_yao.py:59-63, 241-247, 280; dtu.py:80-84, 164-166, 207, 218
//                                                                              jdacs/train.py:269-270
//             or, not centred, what Augmentor.forward returns                  jdacs/models/augmentations.py:20-48
//   imgs_seg  ToTensor -> Normalize(ImageNet)                                  dtu_yao.py:64-67, 237-239; dtu.py:85-86, 160-162
//   filter_mask  the window's mask, at full size or as F.interpolate(scale_factor=0.25) leaves it     train.py:274-275
//
// The reference does this per view on the host with several PIL passes (hue through an HSV round trip) and uploads three fp32
// images.  Here the u8 views are uploaded once and at most three launches, none of which the host waits for, write every tensor:
//
//   sample_prep_stats_kernel      a tile of SP_TILE pixels of one view -> exact integer per-channel sums and sums of squares of the u8
//                                 values, and the fp64 sum of the grey value as it stands in front of the contrast operation
//   sample_prep_aug_stats_kernel  adds the view's grey sums in tile order (the contrast mean), runs the whole chain, writes fp64
//                                 per-channel sums and sums of squares of the x255 result          (only when imgs_aug is centred)
//   sample_prep_write_kernel      adds the view's records in tile order, forms means and deviations in fp64, runs the chain again
//                                 and writes each requested output once
//
// One record of SP_REC_BYTES per (view, tile): 16 slots of 8 bytes -- 0..5 unsigned 64-bit (sum r g b, sum of squares r g b), 6 fp64
// grey sum, 8..13 fp64 (sum r g b, sum of squares r g b of the augmented x255 view); 7, 14, 15 unused.  No atomics: a workgroup sums a
// view's records itself, thread (slot, segment) its sixteenth of the tiles in tile order and one thread per slot the sixteen segment
// sums in order, so a rerun gives the same bits.  Thread t of a tile owns the pixel groups 4 (t + 256 j) .. + 3 whether they are
// fetched as three 32-bit words (tile start 4-byte aligned) or byte by byte, and stores them as float4 or as scalars: alignment
// changes no value.
//
// The per-view parameters (SpView) are HOST data that travel in the kernel arguments, SP_MAXV views to a group of launches.
// Arithmetic is fp32 on values in [0, 1], written as torchvision's tensor formulas are (tests/sample_prep_oracle.py restates it);
// the two centrings subtract and scale in fp64 and round once.

#define SP_TILE 4096          // pixels per workgroup: 16 per thread
#define SP_REC_BYTES 128
#define SP_SLOTS 16
#define SP_MAXV 64            // views per group of launches (their parameters are kernel arguments: 40 bytes each)
#define SP_RAW_SLOTS 0x003Fu
#define SP_GRAY_SLOT 0x0040u
#define SP_AUG_SLOTS 0x3F00u

struct SpView {
    float f[4];               // factors of the four operations, in application order
    float gamma;
    int rect[4];              // y, x, fh, fw of the zeroed window; fh = 0: none
    signed char op[4];        // 0 brightness, 1 contrast, 2 saturation, 3 hue, -1 none
};
struct SpTable { SpView v[SP_MAXV]; };

static __device__ __forceinline__ float sp_clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
static __device__ __forceinline__ float sp_gray(float r, float g, float b) { return 0.299f * r + 0.587f * g + 0.114f * b; }

// rgb -> hsv, h = (h + f) mod 1, hsv -> rgb with colorsys's conventions; a grey pixel (s = 0, h = 0) comes back unchanged
static __device__ __forceinline__ void sp_hue(float& r, float& g, float& b, float f) {
    const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
    if (minc == maxc) return;
    const float d = maxc - minc, s = d / maxc, v = maxc;
    const float rc = (maxc - r) / d, gc = (maxc - g) / d, bc = (maxc - b) / d;
    float h = (r == maxc) ? bc - gc : ((g == maxc) ? 2.0f + rc - bc : 4.0f + gc - rc);
    h = h / 6.0f;
    h -= floorf(h);
    h += f;
    h -= floorf(h);
    const float h6 = h * 6.0f;
    int i = (int)h6;
    const float ff = h6 - (float)i;
    const float p = v * (1.0f - s), q = v * (1.0f - s * ff), t = v * (1.0f - s * (1.0f - ff));
    i = i % 6;
    switch (i) {
        case 0: r = v; g = t; b = p; break;
        case 1: r = q; g = v; b = p; break;
        case 2: r = p; g = v; b = t; break;
        case 3: r = p; g = q; b = v; break;
        case 4: r = t; g = p; b = v; break;
        default: r = v; g = p; b = q; break;
    }
}

// The jitter operations in the view's order.  UP_TO_CONTRAST: stop in front of the contrast operation (the image whose grey mean
// that operation needs).
template <bool UP_TO_CONTRAST>
static __device__ __forceinline__ void sp_jitter(float& r, float& g, float& b, const SpView& v, float cmean) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int op = v.op[k];
        const float f = v.f[k];
        if (op == 0) {
            r = sp_clamp01(f * r); g = sp_clamp01(f * g); b = sp_clamp01(f * b);
        } else if (op == 1) {
            if (UP_TO_CONTRAST) return;
            const float a = (1.0f - f) * cmean;
            r = sp_clamp01(f * r + a); g = sp_clamp01(f * g + a); b = sp_clamp01(f * b + a);
        } else if (op == 2) {
            const float a = (1.0f - f) * sp_gray(r, g, b);
            r = sp_clamp01(f * r + a); g = sp_clamp01(f * g + a); b = sp_clamp01(f * b + a);
        } else if (op == 3) {
            sp_hue(r, g, b, f);
        }
    }
}

// the whole chain on one pixel's u8 values: jitter, gamma (clipped)
static __device__ __forceinline__ void sp_chain(const unsigned (&u)[3], const SpView& v, float cmean, float& r, float& g, float& b) {
    r = (float)u[0] / 255.0f; g = (float)u[1] / 255.0f; b = (float)u[2] / 255.0f;      // ToTensor
    sp_jitter<false>(r, g, b, v, cmean);
    r = sp_clamp01(powf(r, v.gamma)); g = sp_clamp01(powf(g, v.gamma)); b = sp_clamp01(powf(b, v.gamma));
}

// ToPILImage of a float image: x255, truncate (the saturation only guards values outside [0, 1])
static __device__ __forceinline__ unsigned sp_quant(float x) { return (unsigned)fminf(fmaxf(x * 255.0f, 0.0f), 255.0f); }

struct SpSrc {
    const unsigned char* u8;  // kind 0: this view's [H, W, 3] bytes, else null
    const float* f32;         // kind 1: this view's [3, H, W] planes
    int HW;
};

static __device__ __forceinline__ void sp_load1(const SpSrc& s, int p, unsigned (&u)[3]) {
    if (s.u8) {
        u[0] = s.u8[3 * (size_t)p]; u[1] = s.u8[3 * (size_t)p + 1]; u[2] = s.u8[3 * (size_t)p + 2];
    } else {
        u[0] = sp_quant(s.f32[p]); u[1] = sp_quant(s.f32[(size_t)s.HW + p]); u[2] = sp_quant(s.f32[2 * (size_t)s.HW + p]);
    }
}

// Walks the pixels of tile `tile`: fn(p0, cnt, u) with cnt = 4 for a whole group of consecutive pixels p0 .. p0 + 3 and cnt = 1 for
// each of the at most three pixels behind the last whole group.
template <class F>
static __device__ __forceinline__ void sp_walk(const SpSrc& s, int tile, int tid, F fn) {
    const int start = tile * SP_TILE, rest = s.HW - start, n = rest < SP_TILE ? rest : SP_TILE;      // >= 1 by the grid's size
    const int ngroups = n >> 2;
    const bool words = s.u8 && ((((size_t)(s.u8 + 3 * (size_t)start)) & 3) == 0);
    for (int grp = tid; grp < ngroups; grp += 256) {
        const int p0 = start + (grp << 2);
        unsigned u[4][3];
        if (words) {
            const unsigned* wp = reinterpret_cast<const unsigned*>(s.u8 + 3 * (size_t)p0);           // 12 bytes = 4 pixels
            const unsigned w[3] = {wp[0], wp[1], wp[2]};
#pragma unroll
            for (int k = 0; k < 12; ++k) u[k / 3][k % 3] = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) sp_load1(s, p0 + k, u[k]);
        }
        fn(p0, 4, u);
    }
    {
        const int i = (ngroups << 2) + tid;
        if (i < n) {
            unsigned u[4][3] = {};
            sp_load1(s, start + i, u[0]);
            fn(start + i, 1, u);
        }
    }
}

static __device__ __forceinline__ SpSrc sp_view_src(const void* src, int src_kind, long long stride, int HW, int m) {
    SpSrc s;
    s.u8 = src_kind == 0 ? (const unsigned char*)src + (size_t)m * (size_t)stride : nullptr;
    s.f32 = src_kind == 0 ? nullptr : (const float*)src + (size_t)m * (size_t)stride;
    s.HW = HW;
    return s;
}

// Sums the slots named in `mask` over a view's tile records into tot[slot] (LDS, 16 doubles), every sum in tile order: thread
// (slot = tid / 16, segment = tid % 16) adds its sixteenth of the tiles, thread slot < 16 the sixteen segment sums.
static __device__ __forceinline__ void sp_sum_records(const char* __restrict__ recs, int ntiles, unsigned mask, int tid, double* part,
                                                      double* tot) {
    const int slot = tid >> 4, seg = tid & 15;
    const int len = (ntiles + 15) / 16, t0 = seg * len, t1 = (t0 + len < ntiles) ? t0 + len : ntiles;
    double v = 0.0;
    if ((mask >> slot) & 1u) {
        if (slot < 6) {
            unsigned long long a = 0ull;
            for (int t = t0; t < t1; ++t) a += reinterpret_cast<const unsigned long long*>(recs + (size_t)t * SP_REC_BYTES)[slot];
            v = (double)a;                                                              // below 2^53: exact
        } else {
            for (int t = t0; t < t1; ++t) v += reinterpret_cast<const double*>(recs + (size_t)t * SP_REC_BYTES)[slot];
        }
    }
    part[tid] = v;
    __syncthreads();
    if (tid < SP_SLOTS) {
        double a = 0.0;
        for (int k = 0; k < 16; ++k) a += part[tid * 16 + k];
        tot[tid] = a;
    }
    __syncthreads();
}

// launch 1: slots 0..6 of the tile's record
__global__ __launch_bounds__(256) void sample_prep_stats_kernel(const void* __restrict__ src, int src_kind, long long stride,
                                                                SpTable tab, int has_tab, int m0, int HW, char* __restrict__ ws) {
    __shared__ unsigned su[6 * 256];
    __shared__ double sd[256];
    const int tid = threadIdx.x, tile = blockIdx.x, ml = blockIdx.y, m = m0 + ml, ntiles = gridDim.x;
    const SpSrc s = sp_view_src(src, src_kind, stride, HW, m);
    const SpView v = tab.v[ml];
    unsigned a[6] = {0u, 0u, 0u, 0u, 0u, 0u};           // a tile's sums stay below 4096 * 255^2 < 2^32
    double gs = 0.0;
    sp_walk(s, tile, tid, [&](int, int cnt, const unsigned (&u)[4][3]) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt) {
#pragma unroll
                for (int c = 0; c < 3; ++c) { a[c] += u[k][c]; a[3 + c] += u[k][c] * u[k][c]; }
                if (has_tab) {
                    float r = (float)u[k][0] / 255.0f, g = (float)u[k][1] / 255.0f, b = (float)u[k][2] / 255.0f;
                    sp_jitter<true>(r, g, b, v, 0.0f);
                    gs += (double)sp_gray(r, g, b);
                }
            }
    });
#pragma unroll
    for (int f = 0; f < 6; ++f) su[f * 256 + tid] = a[f];
    sd[tid] = gs;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (tid < k) {
#pragma unroll
            for (int f = 0; f < 6; ++f) su[f * 256 + tid] += su[f * 256 + tid + k];
            sd[tid] += sd[tid + k];
        }
        __syncthreads();
    }
    char* rec = ws + ((size_t)m * (size_t)ntiles + (size_t)tile) * SP_REC_BYTES;
    if (tid < 6) reinterpret_cast<unsigned long long*>(rec)[tid] = (unsigned long long)su[tid * 256];
    else if (tid == 6) reinterpret_cast<double*>(rec)[6] = sd[0];
}

// launch 2: slots 8..13 of the tile's record
__global__ __launch_bounds__(256) void sample_prep_aug_stats_kernel(const void* __restrict__ src, int src_kind, long long stride,
                                                                    SpTable tab, int m0, int HW, char* __restrict__ ws) {
    __shared__ double part[256];
    __shared__ double tot[SP_SLOTS];
    __shared__ double sd[6 * 256];
    const int tid = threadIdx.x, tile = blockIdx.x, ml = blockIdx.y, m = m0 + ml, ntiles = gridDim.x;
    const SpSrc s = sp_view_src(src, src_kind, stride, HW, m);
    const SpView v = tab.v[ml];
    char* recs = ws + (size_t)m * (size_t)ntiles * SP_REC_BYTES;
    sp_sum_records(recs, ntiles, SP_GRAY_SLOT, tid, part, tot);
    const float cmean = (float)(tot[6] / (double)HW);
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    sp_walk(s, tile, tid, [&](int, int cnt, const unsigned (&u)[4][3]) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt) {
                float x[3];
                sp_chain(u[k], v, cmean, x[0], x[1], x[2]);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double y = (double)(x[c] * 255.0f);
                    a[c] += y;
                    a[3 + c] += y * y;
                }
            }
    });
#pragma unroll
    for (int f = 0; f < 6; ++f) sd[f * 256 + tid] = a[f];
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (tid < k) {
#pragma unroll
            for (int f = 0; f < 6; ++f) sd[f * 256 + tid] += sd[f * 256 + tid + k];
        }
        __syncthreads();
    }
    if (tid < 6) reinterpret_cast<double*>(recs + (size_t)tile * SP_REC_BYTES)[8 + tid] = sd[tid * 256];
}

struct SpOut {
    float* imgs;
    float* aug;
    float* seg;
    float* fmask;
    int mask_scale, aug_center, channels_last, H, W;
};

// cnt pixels from p0 of view m, three channels each: [M, 3, H, W] planes, or [M, H, W, 3] behind channels_last
static __device__ __forceinline__ void sp_store(float* __restrict__ out, int channels_last, int m, int HW, int p0, int cnt,
                                                const float (&o)[4][3]) {
    if (channels_last) {
        float* q = out + ((size_t)m * (size_t)HW + (size_t)p0) * 3;
        if (cnt == 4 && (((size_t)q) & 15) == 0) {
            float4* q4 = reinterpret_cast<float4*>(q);
            q4[0] = make_float4(o[0][0], o[0][1], o[0][2], o[1][0]);
            q4[1] = make_float4(o[1][1], o[1][2], o[2][0], o[2][1]);
            q4[2] = make_float4(o[2][2], o[3][0], o[3][1], o[3][2]);
        } else {
            for (int k = 0; k < cnt; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) q[3 * k + c] = o[k][c];
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* q = out + ((size_t)m * 3 + c) * (size_t)HW + (size_t)p0;
            if (cnt == 4 && (((size_t)q) & 15) == 0) {
                *reinterpret_cast<float4*>(q) = make_float4(o[0][c], o[1][c], o[2][c], o[3][c]);
            } else {
                for (int k = 0; k < cnt; ++k) q[k] = o[k][c];
            }
        }
    }
}

// launch 3 (launch 2 when imgs_aug is not centred or not asked for)
__global__ __launch_bounds__(256) void sample_prep_write_kernel(const void* __restrict__ src, int src_kind, long long stride,
                                                                SpTable tab, int has_tab, int m0, int HW,
                                                                const char* __restrict__ ws, SpOut out) {
    __shared__ double part[256];
    __shared__ double tot[SP_SLOTS];
    __shared__ double cen[2][3][2];                    // [raw | augmented][channel][mean, 1 / (deviation + 1e-8)]
    const int tid = threadIdx.x, tile = blockIdx.x, ml = blockIdx.y, m = m0 + ml, ntiles = gridDim.x;
    const SpSrc s = sp_view_src(src, src_kind, stride, HW, m);
    const SpView v = tab.v[ml];
    const bool want_aug = has_tab && out.aug, centred = want_aug && out.aug_center;
    const unsigned mask = (out.imgs ? SP_RAW_SLOTS : 0u) | (want_aug ? SP_GRAY_SLOT : 0u) | (centred ? SP_AUG_SLOTS : 0u);
    sp_sum_records(ws + (size_t)m * (size_t)ntiles * SP_REC_BYTES, ntiles, mask, tid, part, tot);
    if (tid < 6) {                                      // center_image: population mean and variance over H W
        const int set = tid / 3, c = tid - 3 * set, base = set * 8;
        const double n = (double)HW, mean = tot[base + c] / n, ex2 = tot[base + 3 + c] / n;
        const double var = ex2 - mean * mean;
        cen[set][c][0] = mean;
        cen[set][c][1] = 1.0 / (sqrt(var > 0.0 ? var : 0.0) + 1e-8);
    }
    __syncthreads();
    const float cmean = (float)(tot[6] / (double)HW);
    const float seg_mean[3] = {0.485f, 0.456f, 0.406f}, seg_std[3] = {0.229f, 0.224f, 0.225f};
    const int W = out.W, sc = out.mask_scale, Hs = out.H / sc, Ws = W / sc;
    const bool need_xy = (want_aug && v.rect[2] > 0) || out.fmask;
    sp_walk(s, tile, tid, [&](int p0, int cnt, const unsigned (&u)[4][3]) {
        float o[4][3];
        if (out.imgs) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) o[k][c] = (float)(((double)u[k][c] - cen[0][c][0]) * cen[0][c][1]);
            sp_store(out.imgs, out.channels_last, m, HW, p0, cnt, o);
        }
        if (out.seg) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) o[k][c] = ((float)u[k][c] / 255.0f - seg_mean[c]) / seg_std[c];
            sp_store(out.seg, out.channels_last, m, HW, p0, cnt, o);
        }
        float wm[4] = {1.0f, 1.0f, 1.0f, 1.0f};
        if (need_xy) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < cnt) {
                    const int p = p0 + k, y = p / W, x = p - y * W;
                    if (v.rect[2] > 0 && y >= v.rect[0] && y < v.rect[0] + v.rect[2] && x >= v.rect[1] && x < v.rect[1] + v.rect[3])
                        wm[k] = 0.0f;
                    if (out.fmask && (y % sc) == 0 && (x % sc) == 0 && y / sc < Hs && x / sc < Ws)
                        out.fmask[((size_t)m * (size_t)Hs + (size_t)(y / sc)) * (size_t)Ws + (size_t)(x / sc)] = wm[k];
                }
        }
        if (want_aug) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k < cnt) {
                    float x[3];
                    sp_chain(u[k], v, cmean, x[0], x[1], x[2]);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float val = centred ? (float)(((double)(x[c] * 255.0f) - cen[1][c][0]) * cen[1][c][1]) : x[c];
                        o[k][c] = val * wm[k];          // the window after the centring (train.py:269-270)
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < 3; ++c) o[k][c] = 0.0f;
                }
            }
            sp_store(out.aug, out.channels_last, m, HW, p0, cnt, o);
        }
    });
}

static long long sp_tiles(long long HW) { return (HW + SP_TILE - 1) / SP_TILE; }

extern "C" long long mvs_sample_prep_workspace_bytes(int M, int H, int W) {
    if (M < 1 || H < 1 || W < 1) return -1;
    if ((long long)M * (long long)H * (long long)W * 3 >= (1ll << 31)) return -1;
    return (long long)M * sp_tiles((long long)H * W) * SP_REC_BYTES;
}

// params, rect: HOST arrays (they are checked here and copied into the kernel arguments)
extern "C" int mvs_sample_prep(const void* src, int src_kind, long long src_image_stride, const float* params, const int* rect,
                               float* imgs, float* imgs_aug, float* imgs_seg, float* filter_mask, int mask_scale, int aug_center,
                               int channels_last, int M, int H, int W, void* ws, hipStream_t stream) {
    MVS_REQUIRE(M >= 1 && H >= 1 && W >= 1, MVS_ERR_SHAPE, "sample_prep: M, H, W >= 1, got %d x %d x %d", M, H, W);
    MVS_REQUIRE((long long)M * (long long)H * (long long)W * 3 < (1ll << 31), MVS_ERR_SHAPE,
                "sample_prep: M * H * W * 3 must stay below 2^31, got %d x %d x %d", M, H, W);
    MVS_REQUIRE(src && ws, MVS_ERR_NULL, "sample_prep: null pointer argument (src or workspace)");
    MVS_REQUIRE(src_kind == 0 || src_kind == 1, MVS_ERR_UNSUPPORTED, "sample_prep: src_kind 0 (u8 HWC) or 1 (fp32 CHW), got %d", src_kind);
    const long long HW = (long long)H * W;
    if (src_image_stride == 0) src_image_stride = 3 * HW;
    MVS_REQUIRE(src_image_stride >= 3 * HW, MVS_ERR_SHAPE, "sample_prep: image stride %lld is less than one image of %lld elements",
                src_image_stride, 3 * HW);
    MVS_REQUIRE(imgs || imgs_aug || imgs_seg || filter_mask, MVS_ERR_NULL, "sample_prep: null pointer argument (every output)");
    MVS_REQUIRE(!imgs_aug || params, MVS_ERR_NULL, "sample_prep: null pointer argument (imgs_aug needs the parameter table)");
    MVS_REQUIRE(!filter_mask || mask_scale == 1 || mask_scale == 4, MVS_ERR_UNSUPPORTED, "sample_prep: mask_scale 1 or 4, got %d",
                mask_scale);
    const int has_tab = (params && imgs_aug) ? 1 : 0;
    for (int m = 0; m < M && has_tab; ++m) {
        const float* p = params + 9 * (size_t)m;
        unsigned seen = 0u;
        for (int k = 0; k < 4; ++k) {
            const float id = p[k];
            MVS_REQUIRE(id == -1.0f || id == 0.0f || id == 1.0f || id == 2.0f || id == 3.0f, MVS_ERR_UNSUPPORTED,
                        "sample_prep: bad operation id %g (view %d, position %d): -1 none, 0 brightness, 1 contrast, 2 saturation, 3 hue",
                        (double)id, m, k);
            if (id >= 0.0f) {
                MVS_REQUIRE(!((seen >> (int)id) & 1u), MVS_ERR_UNSUPPORTED, "sample_prep: operation id %d twice in view %d", (int)id, m);
                seen |= 1u << (int)id;
                MVS_REQUIRE(p[4 + k] == p[4 + k] && p[4 + k] - p[4 + k] == 0.0f, MVS_ERR_UNSUPPORTED,
                            "sample_prep: factor %d of view %d is not finite", k, m);
            }
        }
        MVS_REQUIRE(p[8] > 0.0f && p[8] - p[8] == 0.0f, MVS_ERR_UNSUPPORTED, "sample_prep: gamma must be positive and finite, got %g (view %d)",
                    (double)p[8], m);
    }
    for (int m = 0; m < M && rect; ++m) {
        const int* r = rect + 4 * (size_t)m;
        MVS_REQUIRE(r[2] >= 0 && r[3] >= 0 && r[0] >= 0 && r[1] >= 0 && (long long)r[0] + r[2] <= H && (long long)r[1] + r[3] <= W,
                    MVS_ERR_SHAPE, "sample_prep: window (y %d, x %d, %d x %d) of view %d leaves the %d x %d image", r[0], r[1], r[2], r[3],
                    m, H, W);
    }
    const int ntiles = (int)sp_tiles(HW);
    SpOut out;
    out.imgs = imgs; out.aug = has_tab ? imgs_aug : nullptr; out.seg = imgs_seg; out.fmask = filter_mask;
    out.mask_scale = filter_mask ? mask_scale : 1; out.aug_center = aug_center ? 1 : 0; out.channels_last = channels_last ? 1 : 0;
    out.H = H; out.W = W;
    const bool need_stats = imgs || has_tab;
    for (int m0 = 0; m0 < M; m0 += SP_MAXV) {
        const int mc = M - m0 < SP_MAXV ? M - m0 : SP_MAXV;
        SpTable tab;
        for (int ml = 0; ml < SP_MAXV; ++ml) {
            SpView& v = tab.v[ml];
            const int m = m0 + ml;
            for (int k = 0; k < 4; ++k) {
                v.op[k] = (has_tab && ml < mc) ? (signed char)(int)params[9 * (size_t)m + k] : (signed char)-1;
                v.f[k] = (has_tab && ml < mc) ? params[9 * (size_t)m + 4 + k] : 1.0f;
                v.rect[k] = (rect && ml < mc) ? rect[4 * (size_t)m + k] : 0;
            }
            v.gamma = (has_tab && ml < mc) ? params[9 * (size_t)m + 8] : 1.0f;
        }
        const dim3 grid((unsigned)ntiles, (unsigned)mc);
        int rc;
        if (need_stats) {
            MVS_LAUNCH(sample_prep_stats_kernel, grid, dim3(256), 0, stream, src, src_kind, src_image_stride, tab, has_tab, m0, (int)HW,
                       (char*)ws);
            rc = mvs_check_launch("sample_prep_stats");
            if (rc != MVS_OK) return rc;
        }
        if (has_tab && aug_center) {
            MVS_LAUNCH(sample_prep_aug_stats_kernel, grid, dim3(256), 0, stream, src, src_kind, src_image_stride, tab, m0, (int)HW,
                       (char*)ws);
            rc = mvs_check_launch("sample_prep_aug_stats");
            if (rc != MVS_OK) return rc;
        }
        MVS_LAUNCH(sample_prep_write_kernel, grid, dim3(256), 0, stream, src, src_kind, src_image_stride, tab, has_tab, m0, (int)HW,
                   (const char*)ws, out);
        rc = mvs_check_launch("sample_prep_write");
        if (rc != MVS_OK) return rc;
    }
    return MVS_OK;
}
