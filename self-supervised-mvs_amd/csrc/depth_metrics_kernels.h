// The seven depth-map validation metrics both training scripts log (jdacs/train.py:232-238 and :319-325, jdacs-ms/train.py:271-277),
// all from ONE read of the three maps.  Included by loss.hip; not a translation unit of its own.
//
//   AbsDepthError_metrics, Thres_metrics at T thresholds        jdacs/utils.py:134-163 (the same text in jdacs-ms/utils.py)
//   non_zero_mean_absolute_diff, less_one / less_three          jdacs/losses/unsup_loss.py:86-125, jdacs-ms/losses/unsup_loss.py:89-128
//
// The reference walks the batch in Python with two boolean-mask selections per image and metric (a nonzero + a host synchronisation
// each on a GPU), builds repeat()-ed interval images for the other three, and reads every scalar back with .item(): on the order of a
// hundred tiny launches and ~8 B synchronisations per validation step.  Here:
//
//   depth_metrics_partial_kernel   grid (tiles per image, B), 256 threads: a tile of DM_TILE pixels of one image -> one 64-byte record
//                                  of exact integer counts and fp64 sums of the fp32 per-pixel values (layout below).
//   depth_metrics_finish_kernel    one workgroup: adds every image's records in tile order (16 tiles to a segment, then the segment
//                                  sums in order), forms the outputs by the reference's own fp32 formulas, optionally adds them into a
//                                  running meter (replaces DictAverageMeter + .item()).
//
// No atomics, every sum in a fixed order that does not depend on the addresses: thread t of a tile owns the pixel groups 4 (t + 256 j)
// .. + 3 whether they are fetched as one 16-byte load (est, gt and mask of the image suitably aligned) or as four scalar ones, so a
// bool mask and an fp32 mask, an aligned and an odd-sized image, and two runs all give the same bits.
//
// Semantics kept from the reference (tests/metrics_oracle.py restates them; tests/golden/g16_depth_metrics.npz is the reference's run):
//   * abs error and threshold rates are means per image over the mask, then the mean over images; an empty mask gives 0 / 0 = NaN for
//     the image and for the batch value; '>' is strict;
//   * mae is a SUM over the batch of (sum_pixels / interval_b) / (count_b + 1e-7); less_one / less_three are batch-global,
//     sum / (sum [gt != 0] + 1e-7);
//   * |gt - est| / interval is a true fp32 division before the '<=' test;
//   * every comparison is written in the reference's direction (e > t, q <= k), so a NaN falls where IEEE puts it: a NaN in est at a
//     mask pixel makes the abs error NaN and counts as not above a threshold and not within less_*;
//   * mae multiplies the difference BY the 0/1 mask, fabsf(m * (gt - est)): a NaN or Inf in est at a gt == 0 pixel makes mae NaN (0 * NaN)
//     and leaves the other six values untouched.
// Counts are integers in the kernels and become floats once, at the division.  That equals the reference wherever its fp32 sums of
// ones are exact: BELOW 2^24 PIXELS per sum (per image for the rates and mae, per batch for less_*); 1200 x 1600 is 1.92 M.

#define DM_TILE 4096          // pixels per workgroup: 16 per thread; 128 x 160 -> 5 workgroups per image, 1200 x 1600 -> 469
#define DM_MAXT 8             // thresholds
#define DM_REC_BYTES 64       // one tile record: double s_abs, s_mae; unsigned n_mask, n_thr[8], n_nz, n_le1, n_le3
#define DM_REC_U 12           // unsigned entries of a record (behind the two doubles)
#define DM_FIELDS 14
#define DM_SEG 16             // finish: tiles per segment (one thread adds them, 16 loads in flight)
#define DM_SEGS 256           // finish: segment sums held in LDS per pass
#define DM_IMGS 16            // finish: images per pass (256 threads = 16 images x 16 field slots)

struct DmThres { float t[DM_MAXT]; };

struct DmAcc {
    double s_abs, s_mae;
    unsigned n_mask, n_thr[DM_MAXT], n_nz, n_le1, n_le3;
};

static __device__ __forceinline__ void dm_pixel(float e, float g, bool on, float iv, const DmThres& th, int T, DmAcc& a) {
    if (on) {                                             // utils.py:152-155, :162-163
        const float d = fabsf(e - g);
        a.n_mask += 1u;
        a.s_abs += (double)d;
#pragma unroll
        for (int j = 0; j < DM_MAXT; ++j)
            if (j < T) a.n_thr[j] += (d > th.t[j]) ? 1u : 0u;
    }
    const float m = (g != 0.0f) ? 1.0f : 0.0f;           // unsup_loss.py:90
    a.s_mae += (double)fabsf(m * (g - e));              // :92, literally: 0 * NaN = NaN
    if (g != 0.0f) {
        const float q = fabsf(g - e) / iv;               // :109, a division
        a.n_nz += 1u;
        a.n_le1 += (q <= 1.0f) ? 1u : 0u;
        a.n_le3 += (q <= 3.0f) ? 1u : 0u;
    }
}

// mask: BYTE_MASK ? torch.bool bytes (non-zero = on) : fp32 (> 0.5 = on, the convention of masked_smooth_l1).  interval may be null
// (then iv = NaN: nothing is within less_*, and the finish writes NaN for the three interval metrics anyway).
template <bool BYTE_MASK>
__global__ __launch_bounds__(256) void depth_metrics_partial_kernel(const float* __restrict__ est, const float* __restrict__ gt,
                                                                    const void* __restrict__ mask, const float* __restrict__ interval,
                                                                    DmThres th, int T, int HW, char* __restrict__ ws) {
    __shared__ double sd[2 * 256];
    __shared__ unsigned su[DM_REC_U * 256];
    const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y, ntiles = gridDim.x;
    const size_t base = (size_t)b * (size_t)HW + (size_t)tile * DM_TILE;
    const int rest = HW - tile * DM_TILE, n = rest < DM_TILE ? rest : DM_TILE;       // >= 1 by the grid's size
    const float* e_p = est + base;
    const float* g_p = gt + base;
    const float* mf_p = (const float*)mask + base;
    const unsigned char* mb_p = (const unsigned char*)mask + base;
    const float iv = interval ? interval[b] : __builtin_nanf("");
    const bool vec = ((((size_t)e_p | (size_t)g_p) & 15) == 0) && (BYTE_MASK ? (((size_t)mb_p & 3) == 0) : (((size_t)mf_p & 15) == 0));
    DmAcc a;
    a.s_abs = 0.0; a.s_mae = 0.0; a.n_mask = 0u; a.n_nz = 0u; a.n_le1 = 0u; a.n_le3 = 0u;
#pragma unroll
    for (int j = 0; j < DM_MAXT; ++j) a.n_thr[j] = 0u;
    const int ngroups = n >> 2;
    for (int grp = tid; grp < ngroups; grp += 256) {
        const int i = grp << 2;
        float e[4], g[4];
        bool on[4];
        if (vec) {
            const float4 e4 = *reinterpret_cast<const float4*>(e_p + i);
            const float4 g4 = *reinterpret_cast<const float4*>(g_p + i);
            e[0] = e4.x; e[1] = e4.y; e[2] = e4.z; e[3] = e4.w;
            g[0] = g4.x; g[1] = g4.y; g[2] = g4.z; g[3] = g4.w;
            if (BYTE_MASK) {
                const unsigned mw = *reinterpret_cast<const unsigned*>(mb_p + i);
                on[0] = (mw & 0xffu) != 0u; on[1] = (mw & 0xff00u) != 0u; on[2] = (mw & 0xff0000u) != 0u; on[3] = (mw & 0xff000000u) != 0u;
            } else {
                const float4 m4 = *reinterpret_cast<const float4*>(mf_p + i);
                on[0] = m4.x > 0.5f; on[1] = m4.y > 0.5f; on[2] = m4.z > 0.5f; on[3] = m4.w > 0.5f;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                e[k] = e_p[i + k];
                g[k] = g_p[i + k];
                on[k] = BYTE_MASK ? (mb_p[i + k] != 0) : (mf_p[i + k] > 0.5f);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) dm_pixel(e[k], g[k], on[k], iv, th, T, a);
    }
    {
        const int i = (ngroups << 2) + tid;             // the at most three pixels behind the last whole group
        if (i < n) dm_pixel(e_p[i], g_p[i], BYTE_MASK ? (mb_p[i] != 0) : (mf_p[i] > 0.5f), iv, th, T, a);
    }
    // workgroup sums through LDS, a fixed tree (hip_emul.h has shuffles for float and int only)
    sd[tid] = a.s_abs;
    sd[256 + tid] = a.s_mae;
    su[tid] = a.n_mask;
#pragma unroll
    for (int j = 0; j < DM_MAXT; ++j) su[(1 + j) * 256 + tid] = a.n_thr[j];
    su[9 * 256 + tid] = a.n_nz;
    su[10 * 256 + tid] = a.n_le1;
    su[11 * 256 + tid] = a.n_le3;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (tid < k) {
            sd[tid] += sd[tid + k];
            sd[256 + tid] += sd[256 + tid + k];
#pragma unroll
            for (int f = 0; f < DM_REC_U; ++f) su[f * 256 + tid] += su[f * 256 + tid + k];
        }
        __syncthreads();
    }
    char* rec = ws + ((size_t)b * (size_t)ntiles + (size_t)tile) * DM_REC_BYTES;
    if (tid < 2) reinterpret_cast<double*>(rec)[tid] = sd[tid * 256];
    else if (tid < DM_FIELDS) reinterpret_cast<unsigned*>(rec + 16)[tid - 2] = su[(tid - 2) * 256];
}

// out [4+T]: abs error, the T threshold rates, mae, less_one, less_three.  per_image [B, 2+T]: abs error, the T rates, and the image's
// term of mae.  meter (may be null): fp64 [4+T] running sums of out; meter_count: one 64-bit integer.
// An image's records are added in tile order, DM_SEG tiles to a segment: thread (segment, field) adds its segment's tiles straight
// from the workspace (16 independent loads, one round trip to the L2 the partial kernel just wrote), thread (image, field) then
// adds the image's segment sums in segment order from LDS, and thread 0 forms the outputs image by image.  (Measured: one thread
// per field walking all 469 records of a 1200 x 1600 image through LDS took 35 us, four times the partial kernel.)  Up to
// DM_IMGS images share a pass; an image of more than DM_SEGS segments (4096 tiles) takes several chunks.
__global__ __launch_bounds__(256) void depth_metrics_finish_kernel(const char* __restrict__ ws, const float* __restrict__ interval, int T,
                                                                   int B, int ntiles, float* __restrict__ out,
                                                                   float* __restrict__ per_image, double* __restrict__ meter,
                                                                   long long* __restrict__ meter_count) {
    __shared__ double partd[2 * DM_SEGS];
    __shared__ unsigned partu[DM_REC_U * DM_SEGS];
    __shared__ double totd[DM_IMGS][2];
    __shared__ unsigned long long totu[DM_IMGS][DM_REC_U];
    const int tid = threadIdx.x, f = tid & 15, hi = tid >> 4;
    const int nseg = (ntiles + DM_SEG - 1) / DM_SEG;
    const int G = nseg <= DM_SEGS ? (DM_SEGS / nseg < DM_IMGS ? DM_SEGS / nseg : DM_IMGS) : 1;      // images per pass
    float s_out[1 + DM_MAXT];                   // thread 0: sums over the images, in image order
    float s_mae = 0.0f;
    unsigned long long g_nz = 0ull, g_le1 = 0ull, g_le3 = 0ull;
#pragma unroll
    for (int j = 0; j < 1 + DM_MAXT; ++j) s_out[j] = 0.0f;
    for (int b0 = 0; b0 < B; b0 += G) {
        const int g = B - b0 < G ? B - b0 : G;
        double accd = 0.0;                      // thread (image hi, field f) of the pass
        unsigned long long accu = 0ull;
        for (int s0 = 0; s0 < nseg; s0 += DM_SEGS) {
            const int ns = nseg - s0 < DM_SEGS ? nseg - s0 : DM_SEGS;                                // g * ns <= DM_SEGS
            for (int it = tid; it < g * ns * 16; it += 256) {
                const int seg = it >> 4, bl = seg / ns, s = seg - bl * ns;                           // (it & 15) == f
                if (f < DM_FIELDS) {
                    const char* img = ws + (size_t)(b0 + bl) * (size_t)ntiles * DM_REC_BYTES;
                    const int t0 = (s0 + s) * DM_SEG;
                    double vd = 0.0;
                    unsigned vu = 0u;
#pragma unroll
                    for (int k = 0; k < DM_SEG; ++k) {                                               // a tile past the end: re-read the last one, add 0
                        const int t = t0 + k, tc = t < ntiles ? t : ntiles - 1;
                        const char* rec = img + (size_t)tc * DM_REC_BYTES;
                        if (f < 2) {
                            const double v = reinterpret_cast<const double*>(rec)[f];
                            vd += t < ntiles ? v : 0.0;
                        } else {
                            const unsigned v = reinterpret_cast<const unsigned*>(rec + 16)[f - 2];
                            vu += t < ntiles ? v : 0u;
                        }
                    }
                    if (f < 2) partd[seg * 2 + f] = vd;
                    else partu[seg * DM_REC_U + (f - 2)] = vu;
                }
            }
            __syncthreads();
            if (hi < g && f < DM_FIELDS) {
                if (f < 2) {
                    for (int s = 0; s < ns; ++s) accd += partd[(hi * ns + s) * 2 + f];
                } else {
                    for (int s = 0; s < ns; ++s) accu += partu[(hi * ns + s) * DM_REC_U + (f - 2)];
                }
            }
            __syncthreads();
        }
        if (hi < g && f < DM_FIELDS) {
            if (f < 2) totd[hi][f] = accd;
            else totu[hi][f - 2] = accu;
        }
        __syncthreads();
        if (tid == 0) {
            for (int bl = 0; bl < g; ++bl) {
                const int b = b0 + bl;
                const float n_mask = (float)totu[bl][0];
                const float abs_b = (float)totd[bl][0] / n_mask;               // mean over the selection: 0 / 0 = NaN when it is empty
                s_out[0] += abs_b;
                per_image[(size_t)b * (2 + T)] = abs_b;
#pragma unroll
                for (int j = 0; j < DM_MAXT; ++j)
                    if (j < T) {
                        const float r = (float)totu[bl][1 + j] / n_mask;
                        s_out[1 + j] += r;
                        per_image[(size_t)b * (2 + T) + 1 + j] = r;
                    }
                const float term = interval ? ((float)totd[bl][1] / interval[b]) / ((float)totu[bl][9] + 1e-7f)     // unsup_loss.py:94
                                            : __builtin_nanf("");
                s_mae += term;
                per_image[(size_t)b * (2 + T) + 1 + T] = term;
                g_nz += totu[bl][9];
                g_le1 += totu[bl][10];
                g_le3 += totu[bl][11];
            }
        }
        // totd / totu are rewritten only behind the next pass's barriers
    }
    if (tid == 0) {
        const float nan = __builtin_nanf("");
        auto put = [&](int j, float v) {
            out[j] = v;
            if (meter) meter[j] += (double)v;
        };
#pragma unroll
        for (int j = 0; j < 1 + DM_MAXT; ++j)
            if (j < 1 + T) put(j, s_out[j] / (float)B);                         // torch.stack(results).mean()
        const float denom = (float)g_nz + 1e-7f;                                // unsup_loss.py:105
        put(1 + T, s_mae);
        put(2 + T, interval ? (float)g_le1 / denom : nan);
        put(3 + T, interval ? (float)g_le3 / denom : nan);
        if (meter) meter_count[0] += 1;
    }
}

static long long dm_tiles(int HW) { return ((long long)HW + DM_TILE - 1) / DM_TILE; }

extern "C" long long mvs_depth_metrics_workspace_bytes(int B, int HW, int T) {
    if (B < 1 || B > 65535 || HW < 1 || T < 0 || T > DM_MAXT) return -1;
    return (long long)B * dm_tiles(HW) * DM_REC_BYTES;
}

extern "C" int mvs_depth_metrics(const float* est, const float* gt, const void* mask, int mask_is_byte, const float* interval,
                                 const float* thresholds, int T, int B, int HW, void* ws, float* out, float* per_image, double* meter,
                                 long long* meter_count, hipStream_t stream) {
    MVS_REQUIRE(est && gt && mask && ws && out && per_image, MVS_ERR_NULL, "depth_metrics: null pointer argument");
    MVS_REQUIRE(T >= 0 && T <= DM_MAXT, MVS_ERR_SHAPE, "depth_metrics: 0 <= T <= %d thresholds, got %d", DM_MAXT, T);
    MVS_REQUIRE(T == 0 || thresholds, MVS_ERR_NULL, "depth_metrics: null pointer argument (thresholds, T = %d)", T);
    MVS_REQUIRE(B >= 1 && B <= 65535, MVS_ERR_SHAPE, "depth_metrics: 1 <= B <= 65535, got %d", B);
    MVS_REQUIRE(HW >= 1, MVS_ERR_SHAPE, "depth_metrics: HW >= 1 pixels per image, got %d", HW);
    MVS_REQUIRE(!meter == !meter_count, MVS_ERR_NULL, "depth_metrics: meter and meter_count go together (one of them is null)");
    DmThres th;
    for (int j = 0; j < DM_MAXT; ++j) th.t[j] = j < T ? thresholds[j] : 0.0f;      // a HOST array, copied into the kernel's arguments
    const int ntiles = (int)dm_tiles(HW);
    const dim3 grid((unsigned)ntiles, (unsigned)B);
    if (mask_is_byte) {
        MVS_LAUNCH(depth_metrics_partial_kernel<true>, grid, dim3(256), 0, stream, est, gt, mask, interval, th, T, HW, (char*)ws);
    } else {
        MVS_LAUNCH(depth_metrics_partial_kernel<false>, grid, dim3(256), 0, stream, est, gt, mask, interval, th, T, HW, (char*)ws);
    }
    const int rc = mvs_check_launch("depth_metrics_partial");
    if (rc != MVS_OK) return rc;
    MVS_LAUNCH(depth_metrics_finish_kernel, dim3(1), dim3(256), 0, stream, (const char*)ws, interval, T, B, ntiles, out, per_image, meter,
               meter_count);
    return mvs_check_launch("depth_metrics_finish");
}
