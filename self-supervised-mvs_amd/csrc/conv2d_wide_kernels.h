// Wide 3x3 stride-1 pad-1 forward convolutions (3 or 32..512 input channels, 32..512 output channels), the 2x2 max pool and the
// bilinear resize of a frozen VGG-style trunk (jdacs/models/seg_dff.py: the feature extractor in front of the NMF).  Included by
// conv2d.hip (the emulation build lists its sources by name).  Forward only, fp32 in / out / accumulate.
//
// Implicit GEMM on the 16x16x4 fp32 MFMA over FLATTENED output positions: row p = (n, y, x) of M = N H W, so a 14x14 map fills its
// tiles like a 224x224 one (a tile may hold the end of one image and the start of the next; the staging tests each row's own
// (y, x) against the borders).  K walks steps of 32: step s = (chunk of 32 input channels, tap), chunk-major so that the nine
// shifted reads of a chunk hit the cache; the Cin = 3 arm has ONE step whose k = tap * 3 + ci (27 of 32 used).
//   workgroup = 4 waves = 2 (positions) x 2 (channels); wave tile = MB m-blocks of 16 positions x 2 column tiles of 16 channels
//   t128x64: MB = 4, t64x64: MB = 2 (same code; which one runs is a matter of how many workgroups the launch has)
//   A (positions x 32 k): staged through registers into a double-buffered LDS image, row stride 40 floats (conflict-free
//     ds_read_b128 for the (row = lane & 15, k quad = lane >> 4) read: the sixteen lanes of every service group land on 64
//     different banks); the loads of step s + 1 are in flight while step s is multiplied, one LDS barrier per step
//   B (weights): MFMA-fragment images read from global memory / L2, 16 bytes per lane, one step ahead.  The weight fragment is the
//     MFMA's A operand (as in conv2d_igemm_kernel), so a lane ends with four CONSECUTIVE channels of one position: float4 stores.
// The accumulation order of an output element (steps in order, k in order) does not depend on the tile, so t128x64 and t64x64
// give the same bits.  Split-K (deep, small layers) writes one partial image per K range and a second kernel adds them in a
// fixed order: no atomics anywhere.
#pragma once

#define C2W_LDA 40   // LDS row stride of the position tile, floats

struct Conv2dWideArgs {
    const float* x;      // [M][Cin]
    const float* wp;     // packed weights [step][2][nbp][64][4]
    const float* bias;   // [Cout] or null
    float* y;            // [M][Cout], or the partial images [split][M][Cout] (then without bias / ReLU)
    int H, W, Cin, Cout, M;
    int nbp;             // 16-wide column tiles of the packed image (Cout rounded up to 64)
    int nsteps, split;   // k-steps in all, K ranges (gridDim.z)
    int relu;
};

MVS_HD inline int c2w_nsteps(int Cin) { return Cin == 3 ? 1 : 9 * (Cin / 32); }
MVS_HD inline int c2w_nbp(int Cout) { return (Cout + 63) / 64 * 4; }

// packed image: element j of lane l, half kk of step s, column tile nb holds W[k = 16 kk + 4 (l >> 4) + j][co = 16 nb + (l & 15)];
// k -> input channel chunk * 32 + k of tap s % 9 (s = chunk * 9 + tap), or (tap = k / 3, ci = k % 3) for Cin = 3; zero beyond
// Cout and beyond k = 26.  wcl: the parameter is [Cout][3][3][Cin] in memory (channels-last) instead of [Cout][Cin][3][3].
__global__ __launch_bounds__(256) void conv2d_wide_pack_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cin, int Cout,
                                                               int nbp, int total, int wcl) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int j = idx & 3, lane = (idx >> 2) & 63;
    int t = idx >> 8;
    const int nb = t % nbp; t /= nbp;
    const int kk = t & 1, s = t >> 1;
    const int k = 16 * kk + 4 * (lane >> 4) + j, co = nb * 16 + (lane & 15);
    int tap, ci;
    if (Cin == 3) { tap = k / 3; ci = k % 3; }
    else { tap = s % 9; ci = (s / 9) * 32 + k; }
    float v = 0.f;
    if (co < Cout && tap < 9) v = c2_wt(w, co, ci, Cin, 9, tap, wcl);
    wp[idx] = v;
}

template <int MB, bool CIN3>
__global__ __launch_bounds__(256) void conv2d_wide_kernel(Conv2dWideArgs a) {
    constexpr int BM = 32 * MB, NR = BM / 32;     // positions per workgroup; rows a thread stages (8 threads x float4 per row)
    __shared__ __attribute__((aligned(16))) float At[2][BM * C2W_LDA];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
    const int wm = wave & 1, wn = wave >> 1;
    const int m0 = blockIdx.x * BM, nb0 = blockIdx.y * 4 + wn * 2;
    const int per = (a.nsteps + a.split - 1) / a.split, s0 = blockIdx.z * per, s1 = min(s0 + per, a.nsteps);
    // the rows this thread stages: r = tid / 8 + 32 i, channel quad q = tid % 8; (y, x) of the row's position, y far outside for p >= M
    const int q = tid & 7;
    int py[NR], px[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int p = m0 + (tid >> 3) + 32 * i;
        px[i] = p % a.W;
        py[i] = p < a.M ? (p / a.W) % a.H : -(1 << 20);
    }
    auto load_a = [&](int s, float4 (&v)[NR]) {
        if (CIN3) {
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const int p = m0 + (tid >> 3) + 32 * i;
                float e[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int k = 4 * q + c, tap = k / 3, ci = k % 3, dy = tap / 3 - 1, dx = tap % 3 - 1;
                    e[c] = 0.f;
                    if (tap < 9 && (unsigned)(py[i] + dy) < (unsigned)a.H && (unsigned)(px[i] + dx) < (unsigned)a.W)
                        e[c] = a.x[((size_t)p + dy * a.W + dx) * 3 + ci];
                }
                v[i] = make_float4(e[0], e[1], e[2], e[3]);
            }
        } else {
            const int chunk = s / 9, tap = s % 9, dy = tap / 3 - 1, dx = tap % 3 - 1;
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const int p = m0 + (tid >> 3) + 32 * i;
                v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                if ((unsigned)(py[i] + dy) < (unsigned)a.H && (unsigned)(px[i] + dx) < (unsigned)a.W)
                    v[i] = *reinterpret_cast<const float4*>(a.x + ((size_t)p + dy * a.W + dx) * a.Cin + chunk * 32 + 4 * q);
            }
        }
    };
    auto load_b = [&](int s, float4 (&b)[2][2]) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
                b[kk][nb] = *reinterpret_cast<const float4*>(a.wp + (((size_t)(2 * s + kk) * a.nbp + nb0 + nb) * 64 + lane) * 4);
    };
    auto store_a = [&](int buf, const float4 (&v)[NR]) {
#pragma unroll
        for (int i = 0; i < NR; ++i)
            *reinterpret_cast<float4*>(&At[buf][((tid >> 3) + 32 * i) * C2W_LDA + 4 * q]) = v[i];
    };
    f32x4 acc[MB][2];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) acc[mb][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float4 av[NR], bw[2][2], bn[2][2];
    if (s0 < s1) {
        load_a(s0, av);
        load_b(s0, bw);
        store_a(0, av);
        // "the first weight fragments are here": without it hipcc carries them as outstanding loads into the loop and, unable to count
        // across the back edge, waits for the loads of step s + 1 in front of the first MFMA of step s (no overlap left)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) MVS_PIN4(bw[kk][nb]);
    }
    MVS_LDS_BARRIER();
    auto multiply = [&](int buf) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            float af[MB][4], bf[2][4];
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                const float4 t = *reinterpret_cast<const float4*>(&At[buf][((wm * MB + mb) * 16 + l15) * C2W_LDA + 16 * kk + 4 * g]);
                af[mb][0] = t.x; af[mb][1] = t.y; af[mb][2] = t.z; af[mb][3] = t.w;
            }
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) { bf[nb][0] = bw[kk][nb].x; bf[nb][1] = bw[kk][nb].y; bf[nb][2] = bw[kk][nb].z; bf[nb][3] = bw[kk][nb].w; }
            // j outermost: consecutive MFMAs go to different accumulators (the 16x16x4 form's dependent latency is longer than its issue interval)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) acc[mb][nb] = MVS_MFMA_16x16x4(bf[nb][j], af[mb][j], acc[mb][nb]);
        }
    };
    // every step but the last requests the next step's operands before it multiplies; the last step stands outside the loop, so
    // the loop body has no branch around its loads (with one, hipcc's wait-count bookkeeping treats the previous step's loads as
    // possibly outstanding and waits for the new position loads before it issues the weight loads)
    for (int s = s0; s + 1 < s1; ++s) {
        const int buf = (s - s0) & 1;
        load_a(s + 1, av);
        load_b(s + 1, bn);
        MVS_SCHED_FENCE();        // (hipcc otherwise sinks the weight loads below the MFMAs, to the point where they are needed at once)
        multiply(buf);
        MVS_SCHED_FENCE();
        store_a(buf ^ 1, av);     // last read in step s - 1, which every wave has left (the barrier below)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) bw[kk][nb] = bn[kk][nb];
        MVS_LDS_BARRIER();
    }
    if (s0 < s1) multiply((s1 - 1 - s0) & 1);
    // D: row = 4 g + r -> channel 16 nb + 4 g + r, column = l15 -> position: four consecutive channels of one position per lane
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int p = m0 + (wm * MB + mb) * 16 + l15;
        if (p >= a.M) continue;
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const int co0 = (nb0 + nb) * 16 + 4 * g;
            if (co0 >= a.Cout) continue;          // (Cout is a multiple of 32: a quad is inside or outside as a whole)
            float4 o = make_float4(acc[mb][nb][0], acc[mb][nb][1], acc[mb][nb][2], acc[mb][nb][3]);
            if (a.split == 1) {
                if (a.bias) {
                    const float4 b = *reinterpret_cast<const float4*>(a.bias + co0);
                    o.x += b.x; o.y += b.y; o.z += b.z; o.w += b.w;
                }
                if (a.relu) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
                *reinterpret_cast<float4*>(a.y + (size_t)p * a.Cout + co0) = o;
            } else {
                *reinterpret_cast<float4*>(a.y + ((size_t)blockIdx.z * a.M + p) * a.Cout + co0) = o;
            }
        }
    }
}

// y[i] = relu(bias + part[0][i] + part[1][i] + ... ) -- the partial images of a split-K launch, added in the order of the K ranges
__global__ __launch_bounds__(256) void conv2d_wide_reduce_kernel(const float* __restrict__ part, const float* __restrict__ bias,
                                                                 float* __restrict__ y, long long quads, int Cout, int split, int relu) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= quads) return;
    float4 s = *reinterpret_cast<const float4*>(part + 4 * i);
    for (int k = 1; k < split; ++k) {
        const float4 t = *reinterpret_cast<const float4*>(part + 4 * ((long long)k * quads + i));
        s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
    }
    if (bias) {
        const float4 b = *reinterpret_cast<const float4*>(bias + (int)((4 * i) % Cout));
        s.x += b.x; s.y += b.y; s.z += b.z; s.w += b.w;
    }
    if (relu) { s.x = fmaxf(s.x, 0.f); s.y = fmaxf(s.y, 0.f); s.z = fmaxf(s.z, 0.f); s.w = fmaxf(s.w, 0.f); }
    *reinterpret_cast<float4*>(y + 4 * i) = s;
}

// 2x2 max pool, stride 2, channels-last, floor on odd sizes: [N,H,W,C] -> [N,H/2,W/2,C]; a NaN wins, as in ATen
__device__ __forceinline__ float c2w_max(float a, float b) { return (b > a || b != b) ? b : a; }
__global__ __launch_bounds__(256) void maxpool2x2_cl_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int C,
                                                            long long quads) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= quads) return;
    const int cq = C / 4, Ho = H / 2, Wo = W / 2;
    const int c = (int)(i % cq);
    long long t = i / cq;
    const int ox = (int)(t % Wo); t /= Wo;
    const int oy = (int)(t % Ho);
    const long long n = t / Ho;
    const float* __restrict__ s = x + (((size_t)n * H + 2 * oy) * W + 2 * ox) * C + 4 * c;
    const float4 v0 = *reinterpret_cast<const float4*>(s), v1 = *reinterpret_cast<const float4*>(s + C);
    const float4 v2 = *reinterpret_cast<const float4*>(s + (size_t)W * C), v3 = *reinterpret_cast<const float4*>(s + (size_t)W * C + C);
    float4 o;
    o.x = c2w_max(c2w_max(v0.x, v1.x), c2w_max(v2.x, v3.x));
    o.y = c2w_max(c2w_max(v0.y, v1.y), c2w_max(v2.y, v3.y));
    o.z = c2w_max(c2w_max(v0.z, v1.z), c2w_max(v2.z, v3.z));
    o.w = c2w_max(c2w_max(v0.w, v1.w), c2w_max(v2.w, v3.w));
    *reinterpret_cast<float4*>(y + 4 * i) = o;
}

// bilinear resize by the rule of F.interpolate(mode='bilinear', align_corners=False): x [N,C,H,W] -> y [N,oh,ow,C] (channels-last);
// source coordinate max(0, (o + 0.5) * in / out - 0.5), the four neighbours clamped to the map
__global__ __launch_bounds__(256) void resize_bilinear_cl_kernel(const float* __restrict__ x, float* __restrict__ y, int C, int H, int W,
                                                                 int oh, int ow, float sy, float sx, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    long long t = i / C;
    const int ox = (int)(t % ow); t /= ow;
    const int oy = (int)(t % oh);
    const long long n = t / oh;
    const float fy = fmaxf(sy * ((float)oy + 0.5f) - 0.5f, 0.f), fx = fmaxf(sx * ((float)ox + 0.5f) - 0.5f, 0.f);
    const int y0 = min((int)fy, H - 1), x0 = min((int)fx, W - 1), y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
    const float ly = fy - (float)y0, lx = fx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
    const float* __restrict__ s = x + ((size_t)n * C + c) * H * W;
    y[i] = hy * (hx * s[(size_t)y0 * W + x0] + lx * s[(size_t)y0 * W + x1]) + ly * (hx * s[(size_t)y1 * W + x0] + lx * s[(size_t)y1 * W + x1]);
}
