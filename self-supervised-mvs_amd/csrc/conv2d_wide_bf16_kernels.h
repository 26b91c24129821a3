// OPT-IN arithmetic of the frozen trunk's wide 3x3 convolutions (conv2d_wide_kernels.h): the same implicit GEMM on the bf16 MFMA
// (v_mfma_f32_16x16x32_bf16), fp32 in / out / accumulate.  Chosen per call by the `arith` argument of the mvs_*_arith entries
// (include/mvs_hip.h), never by a process-wide knob: the packed weight image depends on it.
//   MVS_ARITH_BF16 ("bf16"): operands rounded to nearest-even bf16 (the rounding of conv3d_bf16.hip's f2bf, here the hardware's
//     v_cvt_pk_bf16_f32), ONE product, fp32 accumulation: with rounded operands every product is exact, what differs from an fp32
//     convolution of the rounded operands is the order of the accumulation alone.
//   (A second mode, "bf16x3" -- fp32 operands split into three bf16 terms, six products, conv3d_x3.hip's arithmetic -- was built on
//   this kernel and measured: it met the fp32 criterion but did not beat the fp32 trunk, so it is not here.  DESIGN.md section 7.)
// Included by conv2d.hip right after conv2d_wide_kernels.h, whose GEMM view it keeps: rows are flattened positions (n, y, x), a
// tile may span two images and each staged row tests its own (y, x) against the borders; K walks steps of 32 = (chunk of 32 input
// channels, tap), chunk-major; a workgroup is 2 x 2 waves, tiles t128x64 (MB = 4) and t64x64 (MB = 2); the weight fragment is the
// MFMA's A operand, so a lane ends with four consecutive channels of one position (float4 stores); split-K over gridDim.z writes
// partial images that conv2d_wide_reduce_kernel adds in range order; no atomics.  Cin = 3 stays on the fp32 cin3 arm in every mode.
// What differs:
//   * one k-step of 32 is ONE MFMA per 16x16 block: lane (l15 = lane & 15, g = lane >> 4) multiplies k = 8 g .. 8 g + 7, eight
//     consecutive input channels: one 16-byte LDS read for the positions, one 16-byte load for the weights;
//   * positions: loaded as fp32 one step ahead (two float4 = eight channels per item, item = (row, g)), rounded in registers,
//     stored as bf16 into the double-buffered LDS tile.  Row pitch C2WB_PITCH = 6 x 16 bytes (64 used):
//     ds_read_b128 is served in four groups of 16 lanes that mix two k groups, {rows 0-3, 12-15 of g; rows 4-11 of g + 1} and the
//     complement (MI355X LDS table); a lane covers four banks, so a group is conflict-free when its sixteen 16-byte slot numbers
//     row * 6 + g differ mod 16: row * 6 mod 16 walks the EVEN slots with period 8 -- rows {0-3, 12-15} and rows {4-11} each take
//     all eight of them -- and the other k group of the service group sits one slot higher, on the odd ones.  (Pitch 4, unpadded,
//     is 4-way conflicted; pitch 5 collides rows 1-3 of g with rows 5-7 of g + 1.)
//     LDS: t128x64 128 x 96 B x 2 buffers = 24 KB;
//   * weights: rounded ONCE at pack time into a fragment image [step][nbp][64 lanes] x 16 bytes (conv2d_wide_bf_pack_kernel; the
//     parameter contiguous or channels-last, read in place), loaded from L2 one step ahead.
// The position loads are BRANCH-FREE (a position outside the image points at a zero page, as conv3d_x3.hip stages its halo): a
// load under `if (inside)` is a phi with the zero, and hipcc waits for it right there (s_waitcnt vmcnt(0) inside the conditional
// block; seen in this kernel's ISA with the loads under a branch) -- the request "one step ahead" would be an exposed memory
// round trip per k-step.  Measured on the layers no other change touched: 0.082 -> 0.070 ms for 256 -> 256 at 7x56x56.
// The accumulation order of an output (steps in order) does not depend on the tile: t128x64 and t64x64 give
// the same bits; two calls give the same bits.
#pragma once

#define C2WB_PITCH 6   // LDS row pitch of the position tile, 16-byte slots (4 used)

__device__ static __attribute__((aligned(16))) float g_c2wb_zero_page[8];   // what a position outside the image loads

struct Conv2dWideBfArgs {
    const float* x;      // [M][Cin]
    const uint4* wp;     // packed weights [step][nbp][64]
    const float* bias;   // [Cout] or null
    float* y;            // [M][Cout], or the partial images [split][M][Cout] (then without bias / ReLU)
    int H, W, Cin, Cout, M;
    int nbp;             // 16-wide column tiles of the packed image (Cout rounded up to 64)
    int nsteps, split;   // k-steps in all, K ranges (gridDim.z)
    int relu;
};

// eight fp32 -> eight packed bf16, rounded to nearest even
__device__ __forceinline__ uint4 c2wb_round(const float (&v)[8]) {
    return make_uint4(mvs_cvt_pk_bf16(v[0], v[1]), mvs_cvt_pk_bf16(v[2], v[3]), mvs_cvt_pk_bf16(v[4], v[5]), mvs_cvt_pk_bf16(v[6], v[7]));
}

// packed image: lane l of step s, column tile nb holds the eight bf16 W[k = 8 (l >> 4) + j][co = 16 nb + (l & 15)], j = 0..7;
// k -> input channel (s / 9) * 32 + k of tap s % 9; zero beyond Cout.  One thread per (s, nb, l).  wcl: as conv2d_wide_pack_kernel.
__global__ __launch_bounds__(256) void conv2d_wide_bf_pack_kernel(const float* __restrict__ w, uint4* __restrict__ wp, int Cin, int Cout,
                                                                  int nbp, int total, int wcl) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int lane = idx & 63, nb = (idx >> 6) % nbp, s = (idx >> 6) / nbp;
    const int co = nb * 16 + (lane & 15), tap = s % 9, ci0 = (s / 9) * 32 + 8 * (lane >> 4);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = co < Cout ? c2_wt(w, co, ci0 + j, Cin, 9, tap, wcl) : 0.f;
    wp[idx] = c2wb_round(v);
}

template <int MB>
__global__ __launch_bounds__(256) void conv2d_wide_bf_kernel(Conv2dWideBfArgs a) {
    constexpr int BM = 32 * MB, NI = MB / 2;      // positions per workgroup; items (row, k group of 8 channels) a thread stages
    __shared__ __attribute__((aligned(16))) uint4 At[2][BM * C2WB_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
    const int wm = wave & 1, wn = wave >> 1;
    const int m0 = blockIdx.x * BM, nb0 = blockIdx.y * 4 + wn * 2;
    const int per = (a.nsteps + a.split - 1) / a.split, s0 = blockIdx.z * per, s1 = min(s0 + per, a.nsteps);
    // the items this thread stages: row r = tid / 4 + 64 i, k group kq = tid % 4; (y, x) of the row's position, y far outside for p >= M
    const int kq = tid & 3;
    int py[NI], px[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int p = m0 + (tid >> 2) + 64 * i;
        px[i] = p % a.W;
        py[i] = p < a.M ? (p / a.W) % a.H : -(1 << 20);
    }
    auto load_a = [&](int s, float4 (&v)[NI][2]) {
        const int chunk = s / 9, tap = s % 9, dy = tap / 3 - 1, dx = tap % 3 - 1;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int p = m0 + (tid >> 2) + 64 * i;
            const bool inside = (unsigned)(py[i] + dy) < (unsigned)a.H && (unsigned)(px[i] + dx) < (unsigned)a.W;
            const float* src = inside ? a.x + ((size_t)p + dy * a.W + dx) * a.Cin + chunk * 32 + 8 * kq : g_c2wb_zero_page;
            v[i][0] = reinterpret_cast<const float4*>(src)[0];
            v[i][1] = reinterpret_cast<const float4*>(src)[1];
        }
    };
    auto load_b = [&](int s, uint4 (&b)[2]) {
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) b[nb] = a.wp[((size_t)s * a.nbp + nb0 + nb) * 64 + lane];
    };
    auto store_a = [&](int buf, const float4 (&v)[NI][2]) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const float e[8] = {v[i][0].x, v[i][0].y, v[i][0].z, v[i][0].w, v[i][1].x, v[i][1].y, v[i][1].z, v[i][1].w};
            At[buf][((tid >> 2) + 64 * i) * C2WB_PITCH + kq] = c2wb_round(e);
        }
    };
    f32x4 acc[MB][2];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) acc[mb][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float4 av[NI][2];
    uint4 bw[2], bn[2];
    if (s0 < s1) {
        load_a(s0, av);
        load_b(s0, bw);
        store_a(0, av);
        // "the first weight fragments are here" (as conv2d_wide_kernel: keeps their wait out of the loop)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) MVS_PIN4(bw[nb]);
    }
    MVS_LDS_BARRIER();
    auto multiply = [&](int buf) {
        mvs_bf16x8 wf[2], pf[MB];
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) wf[nb] = *reinterpret_cast<const mvs_bf16x8*>(&bw[nb]);
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) pf[mb] = *reinterpret_cast<const mvs_bf16x8*>(&At[buf][((wm * MB + mb) * 16 + l15) * C2WB_PITCH + g]);
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) acc[mb][nb] = MVS_MFMA_16x16x32_BF16(wf[nb], pf[mb], acc[mb][nb]);
    };
    // the loop of conv2d_wide_kernel: every step but the last requests the next step's operands before it multiplies
    for (int s = s0; s + 1 < s1; ++s) {
        const int buf = (s - s0) & 1;
        load_a(s + 1, av);
        load_b(s + 1, bn);
        MVS_SCHED_FENCE();
        multiply(buf);
        MVS_SCHED_FENCE();
        store_a(buf ^ 1, av);     // last read in step s - 1, which every wave has left (the barrier below)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) bw[nb] = bn[nb];
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
