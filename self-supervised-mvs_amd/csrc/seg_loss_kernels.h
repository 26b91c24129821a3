// The co-segmentation loss of JDACS (the "CS" of the name; jdacs/train.py:204, jdacs-ms/train.py:231), fused.  Included by
// unsup_loss.hip (it shares unsup_sample, block_sum and UNSUP_MAXV with the photometric loss); not a translation unit of its own.
//
// 1. NMF solve: replaces NMF + multiplicative_update_step + approximation_error (jdacs/models/seg_dff.py:21-106).  The reference
//    issues about a dozen small launches per iteration and synchronises with the host at every tenth one (the stopping test); here
//    an iteration is two launches and the stopping decision is taken on the device:
//      nmf_rows_kernel    one workgroup per block of NMF_ROWS rows of V: HH = H H^t (recomputed by every workgroup from the 8 KB H,
//                         the same bits everywhere), its rows of W (VH row, W HH row, == 0 -> 1e-7, W *= VH / WHH), and from the SAME
//                         rows of V the workgroup's partial W^t V [k,m], W^t W [k,k] with the new W.  V is read from memory once
//                         per iteration (the second pass over the workgroup's 16 rows hits the cache).
//      nmf_finish_kernel  32 columns of H per workgroup: adds the partial rows in a fixed order, (W^t W) H, == 0 -> 1e-7,
//                         H *= WV / WWH.  Every workgroup also adds the rows' error partials (same order -> same decision in every
//                         workgroup, no communication) and workgroup 0 writes the solve's state.
//    The Frobenius error of the state after iteration t rides in the row launch of iteration t + 1, BEFORE that launch touches W;
//    because the decision is only known once that launch's partials are added, W is double-buffered (launch L reads buffer L & 1 and
//    writes the other one): a solve that stops keeps the buffer the launch read from and leaves H as it is.  The state is
//    double-buffered the same way (launch L reads slot L & 1, workgroup 0 of its finish writes slot (L + 1) & 1), so no workgroup
//    reads what another one of the same launch writes.  Launches enqueued after the stop read `done` and return at once.  Nothing
//    waits on another workgroup; every cross-workgroup sum is per-workgroup partial rows + a fixed-order finish: same bits every run.
//
// 2. Segmentation loss: replaces compute_seg_loss (jdacs/losses/unsup_seg_loss.py:21-34) per source view of UnSupSegLoss.forward
//    (:62-75) with its inverse_warping (jdacs/losses/homography.py:186-351): sample geometry and validity by unsup_sample, logits =
//    the bilinearly warped K segmentation values, target = first maximum of the reference map, mean cross-entropy over the valid
//    pixels of ALL batch items.  Forward: seg_terms_kernel (per-workgroup partial sums / exact counts) -> seg_finish_kernel;
//    backward: one launch, d total / d depth through the sample coordinates only (the maps are constants: seg_dff.py:142).

#define NMF_ROWS 16
#define NMF_STATE 8      // floats per state slot: done, iterations run, e0, e_prev, e_last, non-finite entries of W, buffer that holds W
#define NMF_MAXK 8
#define NMF_EPSILON 1e-7f

struct NmfArgs {
    const float* V;      // [P,n,m]
    float* W;            // [P,n,k]  buffer 0
    float* H;            // [P,k,m]
    float* state;        // ws: [P][2][NMF_STATE]
    float* w1;           // ws: [P,n,k]  buffer 1
    float* pwv;          // ws: [P][nblk][k][m] partial W^t V
    float* pww;          // ws: [P][nblk][k*k]  partial W^t W
    float* pe;           // ws: [P][nblk][2]    partial squared error, non-finite count
    float* status;       // [P,4]
    float tol;
    int n, m, nblk, update_h;
    int launch;          // index of this launch pair
    int update;          // 0: error-only launch (the check after the last iteration)
    int want_err;        // this launch carries the error of the state it reads
};

__host__ __device__ constexpr int nmf_sym(int a, int b, int K) { return a <= b ? a * K - a * (a - 1) / 2 + (b - a) : b * K - b * (b - 1) / 2 + (a - b); }

// Workgroup sums go through LDS in two levels (16 + 16 terms, fixed order) rather than through wave shuffles: one exchange serves
// all rows of the workgroup, and the thread-per-lane CPU emulation pays per exchange.  Row strides 272 / 68 keep both levels free of
// bank conflicts.
constexpr int nmf_max(int a, int b) { return a > b ? a : b; }

template <int K>
__global__ __launch_bounds__(256) void nmf_rows_kernel(NmfArgs a) {
    constexpr int NH = K * (K + 1) / 2;       // upper triangle of HH
    constexpr int RC = NMF_ROWS * K;          // (row, factor) pairs of the workgroup; + 4 rows of per-wave error partials
    __shared__ float buf[nmf_max(NH * 272, (RC + 4) * 68)];
    __shared__ float l1[nmf_max(NH * 16, (RC + 4) * 4)];
    __shared__ float hhs[NH];
    __shared__ float wsh[NMF_ROWS][K];
    __shared__ float badl[RC];
    __shared__ float errw[4];
    const int p = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* __restrict__ st = a.state + ((size_t)p * 2 + (a.launch & 1)) * NMF_STATE;
    if (st[0] != 0.f) return;                       // the solve has stopped: nothing to do
    const int n = a.n, m = a.m;
    const float* __restrict__ V = a.V + (size_t)p * n * m;
    const float* __restrict__ H = a.H + (size_t)p * K * m;
    float* Wb0 = a.W + (size_t)p * n * K;
    float* Wb1 = a.w1 + (size_t)p * n * K;
    const float* __restrict__ Win = (a.launch & 1) ? Wb1 : Wb0;
    float* __restrict__ Wout = (a.launch & 1) ? Wb0 : Wb1;

    // HH = H H^t (upper triangle), the same sum in every workgroup
    if (a.update) {
        float hh[NH];
#pragma unroll
        for (int q = 0; q < NH; ++q) hh[q] = 0.f;
        for (int j = tid; j < m; j += 256) {
            float h[K];
#pragma unroll
            for (int c = 0; c < K; ++c) h[c] = H[(size_t)c * m + j];
#pragma unroll
            for (int c = 0; c < K; ++c)
#pragma unroll
                for (int d = c; d < K; ++d) hh[nmf_sym(c, d, K)] += h[c] * h[d];
        }
#pragma unroll
        for (int q = 0; q < NH; ++q) buf[q * 272 + tid] = hh[q];
        __syncthreads();
        for (int t = tid; t < NH * 16; t += 256) {
            const int q = t >> 4, sg = t & 15;
            float s = 0.f;
            for (int i = 0; i < 16; ++i) s += buf[q * 272 + i * 16 + sg];
            l1[t] = s;
        }
        __syncthreads();
        if (tid < NH) {
            float s = 0.f;
            for (int i = 0; i < 16; ++i) s += l1[tid * 16 + i];
            hhs[tid] = s;
        }
        __syncthreads();
    }

    // phase A: one wave per row, four rows per wave -- V H^t row and the error of the state read; then one thread per (row, factor)
    const int i0 = blk * NMF_ROWS;
    {
        float vh[4][K];
        float err = 0.f;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
#pragma unroll
            for (int c = 0; c < K; ++c) vh[rr][c] = 0.f;
            const int i = i0 + wave + 4 * rr;
            if (i < n) {
                float w[K];
#pragma unroll
                for (int c = 0; c < K; ++c) w[c] = Win[(size_t)i * K + c];
                const float* __restrict__ vr = V + (size_t)i * m;
                for (int j = lane; j < m; j += 64) {
                    const float v = vr[j];
                    float wh = 0.f;
#pragma unroll
                    for (int c = 0; c < K; ++c) {
                        const float h = H[(size_t)c * m + j];
                        vh[rr][c] += v * h;
                        wh += w[c] * h;
                    }
                    if (a.want_err) { const float d = v - wh; err += d * d; }
                }
            }
        }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
#pragma unroll
            for (int c = 0; c < K; ++c) buf[((wave + 4 * rr) * K + c) * 68 + lane] = vh[rr][c];
        buf[(RC + wave) * 68 + lane] = err;
    }
    __syncthreads();
    for (int t = tid; t < (RC + 4) * 4; t += 256) {
        const int rc = t >> 2, sg = t & 3;
        float s = 0.f;
        for (int i = 0; i < 16; ++i) s += buf[rc * 68 + i * 4 + sg];
        l1[t] = s;
    }
    __syncthreads();
    if (tid < RC) {
        const int r = tid / K, c = tid - r * K, i = i0 + r;
        float wn = 0.f, bad = 0.f;
        if (a.update && i < n) {
            const float vh = ((l1[4 * tid] + l1[4 * tid + 1]) + l1[4 * tid + 2]) + l1[4 * tid + 3];
            float whh = 0.f;
#pragma unroll
            for (int d = 0; d < K; ++d) whh += Win[(size_t)i * K + d] * hhs[nmf_sym(d, c, K)];
            if (whh == 0.f) whh = NMF_EPSILON;
            wn = Win[(size_t)i * K + c] * (vh / whh);
            if (!(fabsf(wn) <= 3.402823466e38f)) bad = 1.f;
            Wout[(size_t)i * K + c] = wn;
        }
        wsh[r][c] = wn;
        badl[tid] = bad;
    } else if (tid < RC + 4) {
        errw[tid - RC] = ((l1[4 * tid] + l1[4 * tid + 1]) + l1[4 * tid + 2]) + l1[4 * tid + 3];
    }
    __syncthreads();

    // phase B: the workgroup's partial W^t V and W^t W with the new rows (V rows again: cache hits)
    if (a.update && a.update_h) {
        const int nr = min(NMF_ROWS, n - i0);
        float* __restrict__ pwv = a.pwv + ((size_t)p * a.nblk + blk) * K * m;
        for (int j = tid; j < m; j += 256) {
            float acc[K];
#pragma unroll
            for (int c = 0; c < K; ++c) acc[c] = 0.f;
            for (int r = 0; r < nr; ++r) {
                const float v = V[(size_t)(i0 + r) * m + j];
#pragma unroll
                for (int c = 0; c < K; ++c) acc[c] += wsh[r][c] * v;
            }
#pragma unroll
            for (int c = 0; c < K; ++c) pwv[(size_t)c * m + j] = acc[c];
        }
        if (tid < K * K) {
            const int c = tid / K, d = tid - c * K;
            float s = 0.f;
            for (int r = 0; r < nr; ++r) s += wsh[r][c] * wsh[r][d];
            a.pww[((size_t)p * a.nblk + blk) * K * K + tid] = s;
        }
    }
    if (tid == 255) {
        float nf = 0.f;
        for (int q = 0; q < RC; ++q) nf += badl[q];
        float* pe = a.pe + ((size_t)p * a.nblk + blk) * 2;
        pe[0] = (errw[0] + errw[1]) + (errw[2] + errw[3]);
        pe[1] = nf;
    }
}

template <int K>
__global__ __launch_bounds__(256) void nmf_finish_kernel(NmfArgs a) {
    __shared__ float ebuf[2 * 272];
    __shared__ float el1[32];
    __shared__ float ww4[4][64];
    __shared__ float ww[64];
    __shared__ float wv8[8][K][32];
    __shared__ float hs[K][32];
    const int p = blockIdx.y, tid = threadIdx.x;
    const float* __restrict__ s_in = a.state + ((size_t)p * 2 + (a.launch & 1)) * NMF_STATE;
    float* __restrict__ s_out = a.state + ((size_t)p * 2 + ((a.launch + 1) & 1)) * NMF_STATE;
    if (s_in[0] != 0.f) {                            // stopped earlier: hand the state on, nothing else
        if (blockIdx.x == 0 && tid < NMF_STATE) s_out[tid] = s_in[tid];
        return;
    }
    // the rows' error / non-finite partials, in the same order in every workgroup
    {
        float e0s = 0.f, e1s = 0.f;
        const float* __restrict__ pe = a.pe + (size_t)p * a.nblk * 2;
        for (int b = tid; b < a.nblk; b += 256) { e0s += pe[2 * b]; e1s += pe[2 * b + 1]; }
        ebuf[tid] = e0s;
        ebuf[272 + tid] = e1s;
    }
    __syncthreads();
    if (tid < 32) {
        const int q = tid >> 4, sg = tid & 15;
        float sum = 0.f;
        for (int i = 0; i < 16; ++i) sum += ebuf[q * 272 + i * 16 + sg];
        el1[tid] = sum;
    }
    __syncthreads();
    float e2[2] = {0.f, 0.f};
    for (int i = 0; i < 16; ++i) { e2[0] += el1[i]; e2[1] += el1[16 + i]; }
    bool stop = false;
    float e0 = s_in[2], eprev = s_in[3], elast = s_in[4];
    if (a.want_err) {
        const float e = sqrtf(e2[0]);
        elast = e;
        if (a.launch == 0) { e0 = e; eprev = e; }
        else if (a.update && a.tol > 0.f) {        // seg_dff.py:98-102
            stop = (eprev - e) / e0 < a.tol;
            if (!stop) eprev = e;
        }
    }
    const bool keep = stop || !a.update;            // W, its count and the iteration counter stay what they were
    if (blockIdx.x == 0 && tid == 0) {
        s_out[0] = stop ? 1.f : 0.f;
        s_out[1] = keep ? s_in[1] : (float)(a.launch + 1);
        s_out[2] = e0; s_out[3] = eprev; s_out[4] = elast;
        s_out[5] = keep ? s_in[5] : e2[1];
        s_out[6] = keep ? s_in[6] : (float)((a.launch + 1) & 1);
        s_out[7] = 0.f;
    }
    if (keep || !a.update_h) return;

    // H *= (W^t V) / ((W^t W) H) for 32 columns: 8 slices of the partial rows per column, joined in slice order
    const int m = a.m, nblk = a.nblk;
    const int c = tid & 31, s = tid >> 5, j = blockIdx.x * 32 + c;
    float* __restrict__ H = a.H + (size_t)p * K * m;
    {
        const int chunk = (nblk + 7) / 8, b0 = s * chunk, b1 = min(nblk, b0 + chunk);
        const float* __restrict__ pwv = a.pwv + (size_t)p * nblk * K * m;
        float acc[K];
#pragma unroll
        for (int q = 0; q < K; ++q) acc[q] = 0.f;
        if (j < m)
            for (int b = b0; b < b1; ++b) {
#pragma unroll
                for (int q = 0; q < K; ++q) acc[q] += pwv[((size_t)b * K + q) * m + j];
            }
#pragma unroll
        for (int q = 0; q < K; ++q) wv8[s][q][c] = acc[q];
    }
    {
        const int s4 = tid >> 6, e = tid & 63;
        const int chunk = (nblk + 3) / 4, b0 = s4 * chunk, b1 = min(nblk, b0 + chunk);
        const float* __restrict__ pww = a.pww + (size_t)p * nblk * K * K;
        float t = 0.f;
        if (e < K * K)
            for (int b = b0; b < b1; ++b) t += pww[(size_t)b * K * K + e];
        ww4[s4][e] = t;
    }
    if (s < K) hs[s][c] = j < m ? H[(size_t)s * m + j] : 0.f;
    __syncthreads();
    if (tid < 64) ww[tid] = ((ww4[0][tid] + ww4[1][tid]) + ww4[2][tid]) + ww4[3][tid];
    __syncthreads();
    if (s < K && j < m) {
        float wv = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) wv += wv8[q][s][c];
        float wwh = 0.f;
#pragma unroll
        for (int q = 0; q < K; ++q) wwh += ww[s * K + q] * hs[q][c];
        if (wwh == 0.f) wwh = NMF_EPSILON;
        H[(size_t)s * m + j] = hs[s][c] * (wv / wwh);
    }
}

// the result into the caller's W (when the last accepted buffer is the work space's) and the status row
__global__ __launch_bounds__(256) void nmf_output_kernel(NmfArgs a, int k) {
    const int p = blockIdx.y, idx = blockIdx.x * 256 + threadIdx.x;
    const float* __restrict__ st = a.state + ((size_t)p * 2 + (a.launch & 1)) * NMF_STATE;
    const size_t nk = (size_t)a.n * k;
    if (st[6] != 0.f && (size_t)idx < nk) a.W[(size_t)p * nk + idx] = a.w1[(size_t)p * nk + idx];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        float* o = a.status + (size_t)p * 4;
        o[0] = st[1]; o[1] = st[5]; o[2] = st[2]; o[3] = st[4];
    }
}

static int nmf_shape(int P, int n, int m, int k) {
    MVS_REQUIRE(P >= 1, MVS_ERR_SHAPE, "nmf_solve: needs P >= 1 problems, got P=%d", P);
    MVS_REQUIRE(k >= 1 && k <= NMF_MAXK, MVS_ERR_UNSUPPORTED, "nmf_solve: needs 1 <= k <= %d factors, got k=%d", NMF_MAXK, k);
    MVS_REQUIRE(n >= k && m >= k, MVS_ERR_SHAPE, "nmf_solve: needs n >= k and m >= k, got n=%d m=%d k=%d", n, m, k);
    MVS_REQUIRE((long long)n * m < (1LL << 31), MVS_ERR_SHAPE, "nmf_solve: n*m = %lld must stay below 2^31", (long long)n * m);
    MVS_REQUIRE(P <= 65535, MVS_ERR_SHAPE, "nmf_solve: at most 65535 problems per call (grid y), got P=%d", P);
    return MVS_OK;
}

extern "C" long long mvs_nmf_workspace_floats(int P, int n, int m, int k) {
    if (P < 1 || P > 65535 || k < 1 || k > NMF_MAXK || n < k || m < k || (long long)n * m >= (1LL << 31)) return -1;
    const long long nblk = (n + NMF_ROWS - 1) / NMF_ROWS;
    return (long long)P * (2 * NMF_STATE + (long long)n * k + nblk * k * m + nblk * k * k + nblk * 2);
}

#define NMF_LAUNCH_K(KERNEL, grid)                                                     \
    switch (k) {                                                                       \
        case 1: MVS_LAUNCH(KERNEL<1>, grid, dim3(256), 0, stream, a); break;           \
        case 2: MVS_LAUNCH(KERNEL<2>, grid, dim3(256), 0, stream, a); break;           \
        case 3: MVS_LAUNCH(KERNEL<3>, grid, dim3(256), 0, stream, a); break;           \
        case 4: MVS_LAUNCH(KERNEL<4>, grid, dim3(256), 0, stream, a); break;           \
        case 5: MVS_LAUNCH(KERNEL<5>, grid, dim3(256), 0, stream, a); break;           \
        case 6: MVS_LAUNCH(KERNEL<6>, grid, dim3(256), 0, stream, a); break;           \
        case 7: MVS_LAUNCH(KERNEL<7>, grid, dim3(256), 0, stream, a); break;           \
        default: MVS_LAUNCH(KERNEL<8>, grid, dim3(256), 0, stream, a); break;          \
    }

// 2 launches per iteration + 1 memset + 1 output launch (+ 2 when the last iteration is one the reference tests after)
extern "C" int mvs_nmf_solve(const float* V, float* W, float* H, int P, int n, int m, int k, int update_h, int max_iter, float tol,
                             float* ws, float* status, hipStream_t stream) {
    MVS_REQUIRE(V && W && H && ws && status, MVS_ERR_NULL, "nmf_solve: null pointer argument");
    int rc = nmf_shape(P, n, m, k);
    if (rc) return rc;
    MVS_REQUIRE(max_iter >= 1 && max_iter <= 100000, MVS_ERR_SHAPE, "nmf_solve: needs 1 <= max_iter <= 100000, got %d", max_iter);
    MVS_REQUIRE(tol == tol, MVS_ERR_SHAPE, "nmf_solve: tol is NaN");
    NmfArgs a = NmfArgs{};
    a.V = V; a.W = W; a.H = H; a.status = status; a.tol = tol;
    a.n = n; a.m = m; a.nblk = (n + NMF_ROWS - 1) / NMF_ROWS; a.update_h = update_h ? 1 : 0;
    a.state = ws;
    a.w1 = a.state + (size_t)P * 2 * NMF_STATE;
    a.pwv = a.w1 + (size_t)P * n * k;
    a.pww = a.pwv + (size_t)P * a.nblk * k * m;
    a.pe = a.pww + (size_t)P * a.nblk * k * k;
    if (hipMemsetAsync(a.state, 0, (size_t)P * 2 * NMF_STATE * sizeof(float), stream) != hipSuccess) {
        mvs_set_error("nmf_solve: clearing the solve state failed");
        return MVS_ERR_LAUNCH;
    }
    const dim3 grows(a.nblk, P), gfin(a.update_h ? (m + 31) / 32 : 1, P);
    const bool tail = tol > 0.f && (max_iter - 1) % 10 == 0;      // the test after the last iteration (its outcome changes nothing)
    const int npairs = max_iter + (tail ? 1 : 0);
    for (int L = 0; L < npairs; ++L) {
        a.launch = L;
        a.update = L < max_iter ? 1 : 0;
        a.want_err = (L == 0 || (tol > 0.f && (L - 1) % 10 == 0)) ? 1 : 0;
        NMF_LAUNCH_K(nmf_rows_kernel, grows);
        NMF_LAUNCH_K(nmf_finish_kernel, gfin);
    }
    a.launch = npairs;
    MVS_LAUNCH(nmf_output_kernel, dim3((unsigned)(((long long)n * k + 255) / 256), P), dim3(256), 0, stream, a, k);
    return mvs_check_launch("nmf_solve");
}

// ------------------------------------------------------------------------------------------------
// segmentation loss
// ------------------------------------------------------------------------------------------------
#define SEG_MAXK 8

struct SegArgs {
    const float* ref;                 // [B,H,W,K]
    const float* view[UNSUP_MAXV];    // V x [B,H,W,K]
    const float* kinv;                // [B,9]
    const float* proj;                // [B,V,12]
    const float* depth;               // [B,H,W]
    const float* gout;                // bwd: device scalar d total
    float* part;                      // ws: [V][nblk] partial sums of the per-pixel cross-entropy
    int* cnt;                         // ws: [V][nblk] valid pixels per workgroup (exact)
    int* saved;                       // ws: [16] valid pixels per view
    float* out;                       // fwd: [1+V]
    float* gdepth;                    // bwd: [B,H,W]
    int B, V, H, W, K, nblk;
};

// warped logits of one valid sample, their maximum and the target class (first maximum of the reference map)
__device__ __forceinline__ void seg_logits(const SegArgs& a, const UnsupSample& s, const float* __restrict__ im,
                                           const float* __restrict__ rf, float (&l)[SEG_MAXK], float& mx, int& target) {
    const float wa = s.fx * s.fy, wb = s.fx * (1.0f - s.fy), wc = (1.0f - s.fx) * s.fy, wd = (1.0f - s.fx) * (1.0f - s.fy);
    mx = -3.402823466e38f;
    float best = rf[0];
    target = 0;
#pragma unroll
    for (int c = 0; c < SEG_MAXK; ++c) {
        l[c] = 0.f;
        if (c < a.K) {
            l[c] = wa * im[s.ia + c] + wb * im[s.ib + c] + wc * im[s.ic + c] + wd * im[s.id + c];
            mx = fmaxf(mx, l[c]);
            if (c > 0 && rf[c] > best) { best = rf[c]; target = c; }
        }
    }
}

__global__ __launch_bounds__(256) void seg_terms_kernel(SegArgs a) {
    __shared__ float red[4 * 2];
    const int HW = a.H * a.W, n = a.B * HW;
    const int i = blockIdx.x * 256 + threadIdx.x, v = blockIdx.y;
    float acc[2] = {0.f, 0.f};
    if (i < n) {
        const int b = i / HW, p = i - b * HW, py = p / a.W, px = p - py * a.W;
        const UnsupSample s = unsup_sample(a.kinv + b * 9, a.proj + ((size_t)b * a.V + v) * 12, a.depth[i], px, py, a.H, a.W, a.K);
        if (s.valid > 0.5f) {
            float l[SEG_MAXK], mx;
            int t;
            seg_logits(a, s, a.view[v] + (size_t)b * HW * a.K, a.ref + (size_t)i * a.K, l, mx, t);
            float sum = 0.f, lt = 0.f;
#pragma unroll
            for (int c = 0; c < SEG_MAXK; ++c)
                if (c < a.K) { sum += expf(l[c] - mx); if (c == t) lt = l[c]; }
            acc[0] = -((lt - mx) - logf(sum));      // - log_softmax(logits)[target]
            acc[1] = 1.f;
        }
    }
    block_sum<2>(acc, red);
    if (threadIdx.x == 0) {
        a.part[(size_t)v * a.nblk + blockIdx.x] = acc[0];
        a.cnt[(size_t)v * a.nblk + blockIdx.x] = (int)acc[1];     // <= 256: exact
    }
}

// one workgroup: per view sum / count (0 / 0 = NaN for a view without a valid pixel), then their sum in view order
__global__ __launch_bounds__(256) void seg_finish_kernel(SegArgs a) {
    __shared__ float red[4];
    __shared__ int cred[256];
    __shared__ float term[UNSUP_MAXV];
    const int tid = threadIdx.x;
    for (int v = 0; v < a.V; ++v) {
        float s[1] = {0.f};
        int c = 0;
        for (int k = tid; k < a.nblk; k += 256) { s[0] += a.part[(size_t)v * a.nblk + k]; c += a.cnt[(size_t)v * a.nblk + k]; }
        block_sum<1>(s, red);
        cred[tid] = c;
        __syncthreads();
        if (tid == 0) {
            int t = 0;
            for (int k = 0; k < 256; ++k) t += cred[k];          // integers: exact in any order
            a.saved[v] = t;
            term[v] = s[0] / (float)t;
        }
        __syncthreads();
    }
    if (tid == 0) {
        float total = 0.f;
        for (int v = 0; v < a.V; ++v) { total += term[v]; a.out[1 + v] = term[v]; }
        a.out[0] = total;
    }
}

__global__ __launch_bounds__(256) void seg_grad_depth_kernel(SegArgs a) {
    const int HW = a.H * a.W, n = a.B * HW;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int b = i / HW, p = i - b * HW, py = p / a.W, px = p - py * a.W;
    const float g = a.gout[0];
    float gd = 0.f;
    for (int v = 0; v < a.V; ++v) {
        const int cnt = a.saved[v];
        if (cnt == 0) continue;
        const UnsupSample s = unsup_sample(a.kinv + b * 9, a.proj + ((size_t)b * a.V + v) * 12, a.depth[i], px, py, a.H, a.W, a.K);
        if (!(s.valid > 0.5f)) continue;
        const float* __restrict__ im = a.view[v] + (size_t)b * HW * a.K;
        float l[SEG_MAXK], mx;
        int t;
        seg_logits(a, s, im, a.ref + (size_t)i * a.K, l, mx, t);
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < SEG_MAXK; ++c)
            if (c < a.K) { l[c] = expf(l[c] - mx); sum += l[c]; }
        const float scale = g / (float)cnt;
        float dx = 0.f, dy = 0.f;
#pragma unroll
        for (int c = 0; c < SEG_MAXK; ++c)
            if (c < a.K) {
                const float gl = (l[c] / sum - (c == t ? 1.f : 0.f)) * scale;     // d total / d logit c
                const float pa = im[s.ia + c], pb = im[s.ib + c], pc = im[s.ic + c], pd = im[s.id + c];
                dx += gl * (-(s.fy * pa) - (1.f - s.fy) * pb + s.fy * pc + (1.f - s.fy) * pd);
                dy += gl * (-(s.fx * pa) + s.fx * pb - (1.f - s.fx) * pc + (1.f - s.fx) * pd);
            }
        gd += dx * s.dxdd + dy * s.dydd;
    }
    a.gdepth[i] = gd;
}

static int seg_shape(int B, int V, int H, int W, int K) {
    MVS_REQUIRE(V >= 1 && V <= UNSUP_MAXV, MVS_ERR_UNSUPPORTED, "seg_loss: needs 1 <= V <= %d source views, got V=%d", UNSUP_MAXV, V);
    MVS_REQUIRE(K >= 2 && K <= SEG_MAXK, MVS_ERR_UNSUPPORTED, "seg_loss: needs 2 <= K <= %d segmentation channels, got K=%d", SEG_MAXK, K);
    MVS_REQUIRE(B >= 1, MVS_ERR_SHAPE, "seg_loss: needs B >= 1, got B=%d", B);
    MVS_REQUIRE(H >= 2 && W >= 2, MVS_ERR_SHAPE, "seg_loss: needs H >= 2 and W >= 2, got H=%d W=%d", H, W);
    MVS_REQUIRE((long long)B * H * W * K < (1LL << 31), MVS_ERR_SHAPE, "seg_loss: B*H*W*K = %lld must stay below 2^31 (32-bit offsets)",
                (long long)B * H * W * K);
    return MVS_OK;
}

extern "C" long long mvs_seg_loss_workspace_floats(int B, int V, int H, int W, int K) {
    if (V < 1 || V > UNSUP_MAXV || K < 2 || K > SEG_MAXK || B < 1 || H < 2 || W < 2 || (long long)B * H * W * K >= (1LL << 31)) return -1;
    const long long nblk = ((long long)B * H * W + 255) / 256;
    return 2LL * V * nblk + 16;
}

static int seg_fill(SegArgs& a, const float* ref_seg, const float* const* view_segs, const float* kinv, const float* proj,
                    const float* depth, int B, int V, int H, int W, int K, float* ws) {
    MVS_REQUIRE(ref_seg && view_segs && kinv && proj && depth && ws, MVS_ERR_NULL, "seg_loss: null pointer argument");
    int rc = seg_shape(B, V, H, W, K);
    if (rc) return rc;
    a = SegArgs{};
    a.ref = ref_seg; a.kinv = kinv; a.proj = proj; a.depth = depth;
    for (int v = 0; v < V; ++v) {
        MVS_REQUIRE(view_segs[v], MVS_ERR_NULL, "seg_loss: null view map %d", v);
        a.view[v] = view_segs[v];
    }
    a.B = B; a.V = V; a.H = H; a.W = W; a.K = K;
    a.nblk = (int)(((long long)B * H * W + 255) / 256);
    a.part = ws;
    a.cnt = reinterpret_cast<int*>(ws + (size_t)V * a.nblk);
    a.saved = a.cnt + (size_t)V * a.nblk;
    return MVS_OK;
}

extern "C" int mvs_seg_loss_fwd(const float* ref_seg, const float* const* view_segs, const float* kinv, const float* proj,
                                const float* depth, int B, int V, int H, int W, int K, float* ws, float* out, hipStream_t stream) {
    SegArgs a;
    int rc = seg_fill(a, ref_seg, view_segs, kinv, proj, depth, B, V, H, W, K, ws);
    if (rc) return rc;
    MVS_REQUIRE(out, MVS_ERR_NULL, "seg_loss_fwd: null output");
    a.out = out;
    MVS_LAUNCH(seg_terms_kernel, dim3(a.nblk, V), dim3(256), 0, stream, a);
    MVS_LAUNCH(seg_finish_kernel, dim3(1), dim3(256), 0, stream, a);
    return mvs_check_launch("seg_loss_fwd");
}

extern "C" int mvs_seg_loss_bwd(const float* ref_seg, const float* const* view_segs, const float* kinv, const float* proj,
                                const float* depth, int B, int V, int H, int W, int K, float* ws, const float* grad_out,
                                float* grad_depth, hipStream_t stream) {
    SegArgs a;
    int rc = seg_fill(a, ref_seg, view_segs, kinv, proj, depth, B, V, H, W, K, ws);
    if (rc) return rc;
    MVS_REQUIRE(grad_out && grad_depth, MVS_ERR_NULL, "seg_loss_bwd: null gradient pointer");
    a.gout = grad_out;
    a.gdepth = grad_depth;
    MVS_LAUNCH(seg_grad_depth_kernel, dim3(a.nblk), dim3(256), 0, stream, a);
    return mvs_check_launch("seg_loss_bwd");
}
