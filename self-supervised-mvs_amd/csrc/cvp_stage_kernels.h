// The stage glue of a CVP-MVSNet forward around depth_hypo.hip's kernels (included at the end of that file): what
// CVPMVSNet._forward (jdacs_ms/models/network.py) ran as tiny ATen launches between this library's kernels.
//
//   cvp_cameras_kernel            every camera product of a forward in ONE launch: the conditioned intrinsics of all views and
//                                 levels (conditionIntrinsics), rot / trans of every level's plane sweep (_ms_proj +
//                                 relative_projections), the [B,30] matrices of every refine level (calDepthHypo's host lines:
//                                 three fp64 LU inverses from the solver library and five matmuls), the 48 sweeping planes
//                                 (calSweepingDepthHypo).  One thread per (sample, level) that loops over the views: latency,
//                                 not throughput.  fp64 Gauss-Jordan with partial pivoting; a singular matrix gives inf / nan
//                                 like torch.linalg.inv_ex, no exception.
//   depth_hypo_up_interval_kernel / depth_hypo_up_write_kernel
//                                 the level transition: depth_hypo.hip's two launches reading the COARSE depth map through the
//                                 x2 bilinear up-sampling of F.interpolate(scale_factor=2, align_corners=None), evaluated per fine
//                                 pixel by one inlined function in both launches (same bits), so the up-sampled map is written
//                                 only when the caller wants it.  No atomics, fixed-order sums: two calls give the same bits.
//
// Every product below uses the conditioned intrinsics AS ROUNDED TO fp32 (what in_ms holds, and what the reference's lines read);
// everything after that is fp64 and rounded once on the way out.
#pragma once

#define MVS_CVP_MAX_LEVELS 6     // == MVS_PYRAMID_MAX_LEVELS (pyramid_kernels.h), ops.PYRAMID_MAX_LEVELS
#define MVS_CVP_PLANES 48        // calSweepingDepthHypo's nhypothesis_init

struct CvpCamArgs {
    const float* ref_in;     // [B,3,3]
    const float* src_in;     // [B,S,3,3]
    const float* ref_ex;     // [B,4,4]
    const float* src_ex;     // [B,S,4,4]
    const float* dmin;       // [B] (item 0 is read, like the reference)
    const float* dmax;
    float* in_ms;            // [B,S+1,L,3,3]
    float* rot;              // [L,B,S,3,3]
    float* trans;            // [L,B,S,3]
    double* mats;            // [L-1,B,30] (null when L == 1)
    float* planes;           // [B,48]
    int B, S, L, img_h;
    int level_h[MVS_CVP_MAX_LEVELS];
};

// inverse of the N x N matrix a (row major) into inv: Gauss-Jordan with partial pivoting on [a | I].  Written with constant
// indices after unrolling (the row swap included) so the work matrix stays in registers.
template <int N>
__device__ __forceinline__ void cvp_inverse(const double* a, double* inv) {
    double m[N][2 * N];
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) { m[r][c] = a[r * N + c]; m[r][N + c] = r == c ? 1.0 : 0.0; }
#pragma unroll
    for (int col = 0; col < N; ++col) {
        int piv = col;
        double best = fabs(m[col][col]);
#pragma unroll
        for (int r = col + 1; r < N; ++r) {
            const double v = fabs(m[r][col]);
            if (v > best) { best = v; piv = r; }
        }
#pragma unroll
        for (int r = col + 1; r < N; ++r)
            if (r == piv) {
#pragma unroll
                for (int c = 0; c < 2 * N; ++c) { const double t = m[col][c]; m[col][c] = m[r][c]; m[r][c] = t; }
            }
        const double s = 1.0 / m[col][col];
#pragma unroll
        for (int c = 0; c < 2 * N; ++c) m[col][c] *= s;
#pragma unroll
        for (int r = 0; r < N; ++r) {
            if (r == col) continue;
            const double f = m[r][col];
#pragma unroll
            for (int c = 0; c < 2 * N; ++c) m[r][c] -= f * m[col][c];
        }
    }
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) inv[r * N + c] = m[r][N + c];
}

// K [3,3] fp32 with rows 0 and 1 divided by img_h / level_h, rounded to fp32 (written to out9) and widened again (k)
__device__ __forceinline__ void cvp_condition(const float* __restrict__ K, int img_h, int level_h, float* __restrict__ out9, double* k) {
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        // k * level_h is exact in fp64 (24 + 29 bits at most: the host checks level_h < 2^29), then one rounded division
        const float v = j < 6 ? (float)((double)K[j] * (double)level_h / (double)img_h) : K[j];
        out9[j] = v;
        k[j] = (double)v;
    }
}

// p [4,4] = [k (3x3) * e[:3,:] ; 0 0 0 1]
__device__ __forceinline__ void cvp_proj(const double* k, const double* e, double* p) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) p[r * 4 + c] = (k[r * 3] * e[c] + k[r * 3 + 1] * e[4 + c]) + k[r * 3 + 2] * e[8 + c];
    p[12] = 0.0; p[13] = 0.0; p[14] = 0.0; p[15] = 1.0;
}

__global__ __launch_bounds__(64) void cvp_cameras_kernel(CvpCamArgs a) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.B * a.L) return;
    const int b = i / a.L, l = i - b * a.L, S = a.S, L = a.L;
    const int lh = a.level_h[l];
    double kr[9], er[16], pr[16], pri[16], eri[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) er[j] = (double)a.ref_ex[(size_t)b * 16 + j];
    cvp_condition(a.ref_in + (size_t)b * 9, a.img_h, lh, a.in_ms + (((size_t)b * (S + 1)) * L + l) * 9, kr);
    cvp_proj(kr, er, pr);
    cvp_inverse<4>(pr, pri);
    const bool refine = l < L - 1;            // a level that gets its hypotheses from the level below: [B,30] for depth_hypo.hip
    double* __restrict__ m30 = refine ? a.mats + ((size_t)l * a.B + b) * 30 : nullptr;
    if (refine) {
        cvp_inverse<3>(kr, m30);              // [0..9) K_ref^-1
        cvp_inverse<4>(er, eri);
    }
    for (int s = 0; s < S; ++s) {
        double ks[9], es[16], ps[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) es[j] = (double)a.src_ex[((size_t)b * S + s) * 16 + j];
        cvp_condition(a.src_in + ((size_t)b * S + s) * 9, a.img_h, lh, a.in_ms + (((size_t)b * (S + 1) + s + 1) * L + l) * 9, ks);
        cvp_proj(ks, es, ps);
        float* __restrict__ rot = a.rot + (((size_t)l * a.B + b) * S + s) * 9;
        float* __restrict__ trans = a.trans + (((size_t)l * a.B + b) * S + s) * 3;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) acc += ps[r * 4 + k] * pri[k * 4 + c];
                if (c < 3) rot[r * 3 + c] = (float)acc;
                else trans[r] = (float)acc;
            }
        if (refine && s == 0) {
            // [9..21) T = K_src (E_src E_ref^-1)[:3,:]: the source pixel (homogeneous) of a point in the reference camera's frame
            double rel[12];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    double acc = 0.0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc += es[r * 4 + k] * eri[k * 4 + c];
                    rel[r * 4 + c] = acc;
                }
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    m30[9 + r * 4 + c] = (ks[r * 3] * rel[c] + ks[r * 3 + 1] * rel[4 + c]) + ks[r * 3 + 2] * rel[8 + c];
            // [21..30) A = (K_ref R_ref)(K_src R_src)^-1
            double krr[9], ksr[9], ksri[9];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    krr[r * 3 + c] = (kr[r * 3] * er[c] + kr[r * 3 + 1] * er[4 + c]) + kr[r * 3 + 2] * er[8 + c];
                    ksr[r * 3 + c] = (ks[r * 3] * es[c] + ks[r * 3 + 1] * es[4 + c]) + ks[r * 3 + 2] * es[8 + c];
                }
            cvp_inverse<3>(ksr, ksri);
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    m30[21 + r * 3 + c] = (krr[r * 3] * ksri[c] + krr[r * 3 + 1] * ksri[3 + c]) + krr[r * 3 + 2] * ksri[6 + c];
        }
    }
    if (l == 0) {                             // the coarse level's planes, the same for every sample: batch item 0's range
        const double d0 = (double)a.dmin[0], step = ((double)a.dmax[0] - d0) / (double)(MVS_CVP_PLANES - 1);
        for (int k = 0; k < MVS_CVP_PLANES; ++k) a.planes[(size_t)b * MVS_CVP_PLANES + k] = (float)(d0 + (double)k * step);
    }
}

// Every camera product of one CVPMVSNet forward, one launch (label "cvp_cameras").  level_h: a HOST array of the L level heights
// (level 0 = finest); rows 0 and 1 of every K are divided by img_h / level_h[l].  Outputs: in_ms [B,S+1,L,3,3] (view 0 = reference),
// rot [L,B,S,3,3] / trans [L,B,S,3] of (K_s,l E_s[:3,:] ; 0 0 0 1) (K_ref,l E_ref[:3,:] ; 0 0 0 1)^-1, mats [L-1,B,30] fp64 in the layout
// of this file's header for the levels 0 .. L-2 with source view 0 (may be null when L == 1: nothing is written), planes [B,48].
extern "C" int mvs_cvp_cameras(const float* ref_in, const float* src_in, const float* ref_ex, const float* src_ex, const float* depth_min,
                               const float* depth_max, int B, int S, int L, int img_h, const int* level_h, float* in_ms, float* rot,
                               float* trans, double* mats, float* planes, hipStream_t stream) {
    MVS_REQUIRE(B > 0 && S >= 1 && S <= MVS_MAX_SRC && L >= 1 && L <= MVS_CVP_MAX_LEVELS && img_h > 0 && B <= (1 << 20), MVS_ERR_SHAPE,
                "cvp_cameras: need B >= 1, 1..%d source views, 1..%d levels and a positive image height, got B=%d S=%d L=%d img_h=%d",
                MVS_MAX_SRC, MVS_CVP_MAX_LEVELS, B, S, L, img_h);
    MVS_REQUIRE(ref_in && src_in && ref_ex && src_ex && depth_min && depth_max && level_h && in_ms && rot && trans && planes &&
                (mats || L == 1), MVS_ERR_NULL, "cvp_cameras: null pointer argument");
    CvpCamArgs a = {};
    a.ref_in = ref_in; a.src_in = src_in; a.ref_ex = ref_ex; a.src_ex = src_ex; a.dmin = depth_min; a.dmax = depth_max;
    a.in_ms = in_ms; a.rot = rot; a.trans = trans; a.mats = mats; a.planes = planes;
    a.B = B; a.S = S; a.L = L; a.img_h = img_h;
    for (int l = 0; l < L; ++l) {
        MVS_REQUIRE(level_h[l] > 0 && level_h[l] < (1 << 29), MVS_ERR_SHAPE, "cvp_cameras: level %d has height %d", l, level_h[l]);
        a.level_h[l] = level_h[l];
    }
    MVS_LAUNCH(cvp_cameras_kernel, dim3(mvs_cdiv(B * L, 64)), dim3(64), 0, stream, a);
    return mvs_check_launch("cvp_cameras");
}

// ---- the level transition ---------------------------------------------------------------------------------------------------
struct HypoUpArgs {
    const float* coarse;   // [B,h,w]
    const double* mats;    // [B,30]
    double* part;          // [B][nblk]
    float* hypos;          // [B,8,2h,2w]
    float* depth_up;       // [B,2h,2w] or null
    int B, h, w, nblk;
};

// F.interpolate(scale_factor=2, mode='bilinear', align_corners=None) at fine pixel (y, x) of a [h,w] map: src = (dst + 0.5) / 2 - 0.5
// clamped at 0, the upper neighbour clamped at the last row / column, weights 0 / 0.25 / 0.75 / 1 (exact), combined in ATen's order
// (columns first).  Compiled with -ffp-contract=off like the rest of the library: the same roundings in both launches and builds.
__device__ __forceinline__ float cvp_up2(const float* __restrict__ c, int h, int w, int y, int x) {
    const int y0 = y > 0 ? (y - 1) >> 1 : 0, x0 = x > 0 ? (x - 1) >> 1 : 0;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float ly1 = y > 0 ? ((y & 1) ? 0.25f : 0.75f) : 0.0f, lx1 = x > 0 ? ((x & 1) ? 0.25f : 0.75f) : 0.0f;
    const float ly0 = 1.0f - ly1, lx0 = 1.0f - lx1;
    const float* __restrict__ r0 = c + (size_t)y0 * w;
    const float* __restrict__ r1 = c + (size_t)y1 * w;
    return ly0 * (lx0 * r0[x0] + lx1 * r0[x1]) + ly1 * (lx0 * r1[x0] + lx1 * r1[x1]);
}

__global__ __launch_bounds__(256) void depth_hypo_up_interval_kernel(HypoUpArgs a) {
    __shared__ double red[4];
    const int W = 2 * a.w, HW = 4 * a.h * a.w, b = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const double* __restrict__ m = a.mats + (size_t)b * 30;
    double val = 0.0;
    if (p < HW) {
        const int py = p / W, px = p - py * W;
        const double x = (double)px, y = (double)py, d1 = (double)cvp_up2(a.coarse + (size_t)b * a.h * a.w, a.h, a.w, py, px);
        double u1, v1, z1, u2, v2, z2;
        hypo_project(m, m + 9, x, y, d1, u1, v1, z1);
        hypo_project(m, m + 9, x, y, d1 + 1.0, u2, v2, z2);
        const double theta = atan((v2 - v1) / (u2 - u1));
        const double u3 = u1 + cos(theta), v3 = v1 + sin(theta);          // one pixel along the epipolar line
        const double* __restrict__ A = m + 21;
        const double t1y = z1 * (A[3] * u1 + A[4] * v1 + A[5]), t1z = z1 * (A[6] * u1 + A[7] * v1 + A[8]);
        const double t2y = A[3] * u3 + A[4] * v3 + A[5], t2z = A[6] * u3 + A[7] * v3 + A[8];
        val = fabs((t2z * t1y - t2y * t1z) / (y * t2z - t2y));             // depth_hypo_interval_kernel's closed form
    }
    // deterministic workgroup sum, as in depth_hypo_interval_kernel
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float hi = (float)val, lo = (float)(val - (double)hi);
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const double o = (double)__shfl_xor(hi, s) + (double)__shfl_xor(lo, s);
        val += o;
        hi = (float)val;
        lo = (float)(val - (double)hi);
    }
    if (lane == 0) red[wave] = val;
    __syncthreads();
    if (threadIdx.x == 0) a.part[(size_t)b * a.nblk + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void depth_hypo_up_write_kernel(HypoUpArgs a) {
    __shared__ double interval;
    const int W = 2 * a.w, HW = 4 * a.h * a.w, b = blockIdx.y;
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < a.nblk; ++k) s += a.part[(size_t)b * a.nblk + k];   // same order in every workgroup
        interval = s / (double)HW;
    }
    __syncthreads();
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const int py = p / W, px = p - py * W;
    const float up = cvp_up2(a.coarse + (size_t)b * a.h * a.w, a.h, a.w, py, px);
    if (a.depth_up) a.depth_up[(size_t)b * HW + p] = up;
    const double d1 = (double)up;
#pragma unroll
    for (int k = 0; k < 8; ++k) a.hypos[((size_t)b * 8 + k) * HW + p] = (float)(d1 + (double)(k - 4) * interval);
}

// The transition to the next finer level: depth [B,h,w] fp32 of the coarser level, mats [B,30] fp64 of the finer one, ws: fp64
// scratch of mvs_depth_hypo_workspace_doubles(B, 2h, 2w) values -> hypos [B,8,2h,2w] = up + (k - 4) * interval_b and, when depth_up
// is not null, the up-sampled map [B,2h,2w] itself.  Two launches, labels "depth_hypo_up_interval" and "depth_hypo_up_write".
extern "C" int mvs_depth_hypo_up(const float* depth, const double* mats, int B, int h, int w, double* ws, float* hypos, float* depth_up,
                                 hipStream_t stream) {
    MVS_REQUIRE(depth && mats && ws && hypos, MVS_ERR_NULL, "depth_hypo_up: null pointer argument");
    MVS_REQUIRE(B > 0 && h > 0 && w > 0 && (long long)h * w <= (1 << 28) && B <= 65535, MVS_ERR_SHAPE,
                "depth_hypo_up: bad shape B=%d h=%d w=%d (at most 2^28 coarse pixels, 65535 samples)", B, h, w);
    HypoUpArgs a;
    a.coarse = depth; a.mats = mats; a.part = ws; a.hypos = hypos; a.depth_up = depth_up; a.B = B; a.h = h; a.w = w;
    a.nblk = (4 * h * w + 255) / 256;
    MVS_LAUNCH(depth_hypo_up_interval_kernel, dim3(a.nblk, B), dim3(256), 0, stream, a);
    const int rc = mvs_check_launch("depth_hypo_up_interval");
    if (rc != MVS_OK) return rc;
    MVS_LAUNCH(depth_hypo_up_write_kernel, dim3(a.nblk, B), dim3(256), 0, stream, a);
    return mvs_check_launch("depth_hypo_up_write");
}
