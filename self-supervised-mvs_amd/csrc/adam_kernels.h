// The optimiser step both training scripts build (jdacs/train.py:71, jdacs-ms/train.py:101: optim.Adam(model.parameters(), lr,
// betas=(0.9, 0.999), weight_decay=wd)) as ONE launch over the flat parameter store of dist.FlatGradBucket(flatten_params=True).
// Included by loss.hip; not a translation unit of its own.
//
//   adam_flat_kernel    p, m, v and grad are flat [n]: the path behind a collective (grad = the packed bucket) and under graph capture.
//   adam_table_kernel   the same update, the gradient of flat range [off_k, off_k + n_k) read from its own pointer g_k -- the
//                       parameters' .grad tensors where autograd left them: no gather, no copy.  The table travels BY VALUE in the
//                       kernel arguments (MVS_ADAM_MAX_SEGMENTS x 16 bytes = 2 KB), so there is no upload in front of the launch.
//
// Both are pure streaming (28 bytes per element; 338 k elements for MVSNet, launch-latency bound): a workgroup of 256 threads owns one
// fixed chunk of MVS_ADAM_CHUNK = 1024 flat elements -> 331 workgroups for MVSNet, 1.3 per CU.  Both go through ONE update function
// and ONE range walker (adam_range), so the same (p, m, v, g) values give the same bits on either path whatever the access width
// (-ffp-contract=off in both Makefiles: no fused multiply-add is formed behind the source's back).
//
// Access width is chosen per range from the ACTUAL addresses: p, m and v move as 16-byte accesses when their three addresses are
// congruent mod 16 (scalar head up to the first 16-byte boundary, scalar tail behind the last whole group); the gradient joins with a
// 16-byte load when its address is congruent too and with four 4-byte loads otherwise.  Flat offsets are arbitrary (the prob layer's
// one-element bias makes every later offset odd), so in most table segments g_k is misaligned relative to p: never assumed.
//
// Step counter: ctr[0] = steps taken (t = ctr[0] + 1 is this step's), ctr[1] = a ticket that is 0 between launches.  Every workgroup
// reads ctr[0], does its work, and only then takes a ticket; the workgroup that draws the last one writes ctr[0] = t and ticket = 0.
// So the counter advances by exactly 1 per call, by one lane, after every workgroup has read it -- nobody waits for anybody (no
// grid-wide spinning), it is one launch, and a captured launch stays correct on replay (nothing about t is baked into the arguments).
// The bias corrections 1 - b^t, lr / bc1 and 1 / sqrt(bc2) are formed in fp64 from the doubles the entry received and rounded to fp32
// once; 1 - beta1 and 1 - beta2 are formed in fp64 on the host and rounded once (formed in fp32, 1 - 0.999f is off by 2e-5 relative
// and exp_avg_sq ends 30x less accurate than torch's).

#define MVS_ADAM_CHUNK 1024          // flat elements per workgroup: one 16-byte group per thread
#define MVS_ADAM_MAX_SEGMENTS 128    // table rows per launch: MVSNet has 55 trainable tensors (67 with the refine net), CVP-MVSNet 50

#if defined(MVS_CPU_EMUL)
#define MVS_ADAM_TICKET(ptr) __atomic_fetch_add((ptr), 1, __ATOMIC_RELAXED)
#define MVS_ADAM_PUT(ptr, v) __atomic_store_n((ptr), (v), __ATOMIC_RELAXED)
#else
#define MVS_ADAM_TICKET(ptr) __hip_atomic_fetch_add((ptr), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define MVS_ADAM_PUT(ptr, v) __hip_atomic_store((ptr), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#endif

struct AdamHyper {                   // as the entry received them
    double lr, beta1, beta2;
    float one_minus_b1, b2, one_minus_b2, eps, wd, grad_scale;
};

struct AdamConst {                   // this step's fp32 constants
    float step_size, inv_sqrt_bc2, one_minus_b1, b2, one_minus_b2, eps, wd, grad_scale;
};

struct AdamTable {
    const float* g[MVS_ADAM_MAX_SEGMENTS];
    int off[MVS_ADAM_MAX_SEGMENTS];
    int cnt[MVS_ADAM_MAX_SEGMENTS];
};

static __device__ __forceinline__ AdamConst adam_consts(const AdamHyper& h, int t) {
    const double bc1 = 1.0 - pow(h.beta1, (double)t), bc2 = 1.0 - pow(h.beta2, (double)t);
    AdamConst c;
    c.step_size = (float)(h.lr / bc1);
    c.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    c.one_minus_b1 = h.one_minus_b1;
    c.b2 = h.b2;
    c.one_minus_b2 = h.one_minus_b2;
    c.eps = h.eps;
    c.wd = h.wd;
    c.grad_scale = h.grad_scale;
    return c;
}

// torch.optim.Adam's single-tensor update (L2 weight decay, lerp for exp_avg), everything fp32
static __device__ inline void adam_update(float& p, float& m, float& v, float grad, const AdamConst& c) {
    float g = grad * c.grad_scale;
    if (c.wd != 0.0f) g += c.wd * p;
    m = m + c.one_minus_b1 * (g - m);
    v = c.b2 * v + c.one_minus_b2 * g * g;
    p -= c.step_size * m / (sqrtf(v) * c.inv_sqrt_bc2 + c.eps);
}

// flat elements [lo, hi) of p / m / v, the gradient of element i at g[i - goff] (g == nullptr: zero).  Every thread of the workgroup
// calls it with the same arguments.
static __device__ inline void adam_range(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, const float* __restrict__ g,
                                         int goff, int lo, int hi, const AdamConst& c, int tid) {
    const size_t ap = (size_t)(p + lo) & 15, am = (size_t)(m + lo) & 15, av = (size_t)(v + lo) & 15;
    if (ap != am || ap != av) {                          // p, m, v disagree mod 16: 4-byte accesses throughout
        for (int i = lo + tid; i < hi; i += 256) {
            float pi = p[i], mi = m[i], vi = v[i];
            adam_update(pi, mi, vi, g ? g[i - goff] : 0.0f, c);
            p[i] = pi; m[i] = mi; v[i] = vi;
        }
        return;
    }
    int head = (int)(((16 - ap) & 15) >> 2);            // elements in front of the first 16-byte boundary
    if (head > hi - lo) head = hi - lo;
    const int first = lo + head, ngroups = (hi - first) >> 2, rest = first + (ngroups << 2);
    const bool gvec = g && (((size_t)(g + (first - goff)) & 15) == 0);
    for (int grp = tid; grp < ngroups; grp += 256) {
        const int i = first + (grp << 2);
        float4 p4 = *reinterpret_cast<const float4*>(p + i);
        float4 m4 = *reinterpret_cast<const float4*>(m + i);
        float4 v4 = *reinterpret_cast<const float4*>(v + i);
        float4 g4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (gvec) {
            g4 = *reinterpret_cast<const float4*>(g + (i - goff));
        } else if (g) {
            const float* gi = g + (i - goff);
            g4 = make_float4(gi[0], gi[1], gi[2], gi[3]);
        }
        adam_update(p4.x, m4.x, v4.x, g4.x, c);
        adam_update(p4.y, m4.y, v4.y, g4.y, c);
        adam_update(p4.z, m4.z, v4.z, g4.z, c);
        adam_update(p4.w, m4.w, v4.w, g4.w, c);
        *reinterpret_cast<float4*>(p + i) = p4;
        *reinterpret_cast<float4*>(m + i) = m4;
        *reinterpret_cast<float4*>(v + i) = v4;
    }
    // at most three elements in front and three behind: threads 0..2 and 3..5
    const int i = tid < 3 ? lo + tid : rest + (tid - 3);
    if (tid < 3 ? i < first : (tid < 6 && i < hi)) {
        float pi = p[i], mi = m[i], vi = v[i];
        adam_update(pi, mi, vi, g ? g[i - goff] : 0.0f, c);
        p[i] = pi; m[i] = mi; v[i] = vi;
    }
}

// after the workgroup's last use of t: the workgroup that draws the last ticket advances the counter.  The ticket is a RELAXED
// agent-scope atomic on purpose: a release here would write back the XCD's L2 once per workgroup, and nothing needs it -- the
// workgroup's load of ctr[0] has returned (its value went into every store in front of the barrier) before the ticket is issued,
// p / m / v are read by later launches only, and the counter itself is written and re-read across a launch boundary.
static __device__ __forceinline__ void adam_advance(int* __restrict__ ctr, int t, int tid) {
    __syncthreads();
    if (tid == 0) {
        const int ticket = MVS_ADAM_TICKET(ctr + 1);
        if (ticket == (int)gridDim.x - 1) {
            MVS_ADAM_PUT(ctr, t);
            MVS_ADAM_PUT(ctr + 1, 0);
        }
    }
}

__global__ __launch_bounds__(256) void adam_flat_kernel(float* __restrict__ p, const float* __restrict__ grad, float* __restrict__ m,
                                                        float* __restrict__ v, int n, int* __restrict__ ctr, AdamHyper h) {
    const int tid = threadIdx.x, t = ctr[0] + 1;
    const AdamConst c = adam_consts(h, t);
    const int lo = (int)blockIdx.x * MVS_ADAM_CHUNK, hi = n - lo < MVS_ADAM_CHUNK ? n : lo + MVS_ADAM_CHUNK;
    adam_range(p, m, v, grad, 0, lo, hi, c, tid);
    adam_advance(ctr, t, tid);
}

// workgroup b owns chunk chunk0 + b and walks the rows of the table that overlap it (rows sorted by offset, disjoint: checked by the
// entry).  Elements no row covers are left alone.  advance: 0 for all but the last launch of a table of more than
// MVS_ADAM_MAX_SEGMENTS rows.
__global__ __launch_bounds__(256) void adam_table_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, int nseg,
                                                         int chunk0, int advance, int* __restrict__ ctr, AdamHyper h, AdamTable tab) {
    const int tid = threadIdx.x, t = ctr[0] + 1;
    const AdamConst c = adam_consts(h, t);
    const int lo = (chunk0 + (int)blockIdx.x) * MVS_ADAM_CHUNK, hi = lo + MVS_ADAM_CHUNK;
    int a = 0, b = nseg;                                 // first row that ends behind lo
    while (a < b) {
        const int mid = (a + b) >> 1;
        if (tab.off[mid] + tab.cnt[mid] > lo) b = mid; else a = mid + 1;
    }
    for (int k = a; k < nseg; ++k) {
        const int off = tab.off[k];
        if (off >= hi) break;
        const int end = off + tab.cnt[k];
        adam_range(p, m, v, tab.g[k], off, off > lo ? off : lo, end < hi ? end : hi, c, tid);
    }
    if (advance) adam_advance(ctr, t, tid);
}

#define MVS_ADAM_MAX_N (0x7fffffffLL - 2 * MVS_ADAM_CHUNK)     // flat indices are 32-bit in the kernels, a chunk past the end included

static bool adam_finite(double x) { return x - x == 0.0; }      // false for NaN and +-Inf

static int adam_hyper(const char* who, double lr, double beta1, double beta2, double eps, double wd, double grad_scale, AdamHyper* h) {
    MVS_REQUIRE(adam_finite(lr) && adam_finite(beta1) && adam_finite(beta2) && adam_finite(eps) && adam_finite(wd) && adam_finite(grad_scale),
                MVS_ERR_SHAPE, "%s: non-finite hyper-parameter (lr %g, betas %g %g, eps %g, weight_decay %g, grad_scale %g)", who, lr, beta1,
                beta2, eps, wd, grad_scale);
    MVS_REQUIRE(lr >= 0.0, MVS_ERR_SHAPE, "%s: lr >= 0 required, got %g", who, lr);
    MVS_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, MVS_ERR_SHAPE, "%s: betas in [0, 1) required, got %g %g", who,
                beta1, beta2);
    MVS_REQUIRE(eps >= 0.0, MVS_ERR_SHAPE, "%s: eps >= 0 required, got %g", who, eps);
    MVS_REQUIRE(wd >= 0.0, MVS_ERR_SHAPE, "%s: weight_decay >= 0 required, got %g", who, wd);
    h->lr = lr;
    h->beta1 = beta1;
    h->beta2 = beta2;
    h->one_minus_b1 = (float)(1.0 - beta1);              // fp64, rounded once
    h->b2 = (float)beta2;
    h->one_minus_b2 = (float)(1.0 - beta2);
    h->eps = (float)eps;
    h->wd = (float)wd;
    h->grad_scale = (float)grad_scale;
    return MVS_OK;
}

extern "C" int mvs_adam_limits(int* chunk, int* max_segments) {
    MVS_REQUIRE(chunk && max_segments, MVS_ERR_NULL, "adam_limits: null pointer argument");
    *chunk = MVS_ADAM_CHUNK;
    *max_segments = MVS_ADAM_MAX_SEGMENTS;
    return MVS_OK;
}

extern "C" int mvs_adam_step(float* p, const float* grad, float* m, float* v, long long n, int* step_counter, double lr, double beta1,
                             double beta2, double eps, double weight_decay, double grad_scale, hipStream_t stream) {
    MVS_REQUIRE(p && grad && m && v && step_counter, MVS_ERR_NULL, "adam_step: null pointer argument");
    MVS_REQUIRE(n > 0, MVS_ERR_SHAPE, "adam_step: n > 0 elements required, got %lld", n);
    MVS_REQUIRE(n <= MVS_ADAM_MAX_N, MVS_ERR_UNSUPPORTED, "adam_step: n = %lld elements, at most %lld are served", n, (long long)MVS_ADAM_MAX_N);
    AdamHyper h;
    const int rc = adam_hyper("adam_step", lr, beta1, beta2, eps, weight_decay, grad_scale, &h);
    if (rc != MVS_OK) return rc;
    const unsigned grid = (unsigned)((n + MVS_ADAM_CHUNK - 1) / MVS_ADAM_CHUNK);
    MVS_LAUNCH(adam_flat_kernel, dim3(grid), dim3(256), 0, stream, p, grad, m, v, (int)n, step_counter, h);
    return mvs_check_launch("adam_flat");
}

extern "C" int mvs_adam_step_table(float* p, float* m, float* v, long long n, const float* const* grads, const long long* offsets,
                                   const long long* counts, int nseg, int* step_counter, double lr, double beta1, double beta2,
                                   double eps, double weight_decay, double grad_scale, hipStream_t stream) {
    MVS_REQUIRE(p && m && v && grads && offsets && counts && step_counter, MVS_ERR_NULL, "adam_step_table: null pointer argument");
    MVS_REQUIRE(n > 0, MVS_ERR_SHAPE, "adam_step_table: n > 0 elements required, got %lld", n);
    MVS_REQUIRE(n <= MVS_ADAM_MAX_N, MVS_ERR_UNSUPPORTED, "adam_step_table: n = %lld elements, at most %lld are served", n,
                (long long)MVS_ADAM_MAX_N);
    MVS_REQUIRE(nseg >= 1, MVS_ERR_SHAPE, "adam_step_table: at least one segment required, got %d", nseg);
    long long prev_end = 0;
    for (int k = 0; k < nseg; ++k) {
        MVS_REQUIRE(counts[k] >= 1 && offsets[k] >= 0 && offsets[k] <= n - counts[k], MVS_ERR_SHAPE,
                    "adam_step_table: segment %d = [%lld, +%lld) is empty or falls outside [0, %lld)", k, offsets[k], counts[k], n);
        MVS_REQUIRE(offsets[k] >= prev_end, MVS_ERR_SHAPE,
                    "adam_step_table: segment %d starts at %lld, in front of the end %lld of segment %d (segments must be sorted and disjoint)",
                    k, offsets[k], prev_end, k - 1);
        prev_end = offsets[k] + counts[k];
    }
    AdamHyper h;
    const int rc = adam_hyper("adam_step_table", lr, beta1, beta2, eps, weight_decay, grad_scale, &h);
    if (rc != MVS_OK) return rc;
    for (int k0 = 0; k0 < nseg; k0 += MVS_ADAM_MAX_SEGMENTS) {
        const int ns = nseg - k0 < MVS_ADAM_MAX_SEGMENTS ? nseg - k0 : MVS_ADAM_MAX_SEGMENTS;
        AdamTable tab;
        for (int k = 0; k < MVS_ADAM_MAX_SEGMENTS; ++k) {
            tab.g[k] = k < ns ? grads[k0 + k] : nullptr;
            tab.off[k] = k < ns ? (int)offsets[k0 + k] : 0;
            tab.cnt[k] = k < ns ? (int)counts[k0 + k] : 0;
        }
        const long long c0 = offsets[k0] / MVS_ADAM_CHUNK;
        const long long c1 = (offsets[k0 + ns - 1] + counts[k0 + ns - 1] + MVS_ADAM_CHUNK - 1) / MVS_ADAM_CHUNK;
        const int last = k0 + ns == nseg;
        MVS_LAUNCH(adam_table_kernel, dim3((unsigned)(c1 - c0)), dim3(256), 0, stream, p, m, v, ns, (int)c0, last, step_counter, h, tab);
        const int rcl = mvs_check_launch(last ? "adam_table" : "adam_table part");
        if (rcl != MVS_OK) return rcl;
    }
    return MVS_OK;
}
