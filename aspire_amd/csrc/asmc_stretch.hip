// asmc_stretch.hip — the affine-invariant ensemble "stretch" move (Goodman & Weare 2010; emcee's default StretchMove on a
// RedBlueMove with nsplits = 2, randomize_split = True) as the mutation of the "emcee_smc" sampler (reference
// src/aspire/samplers/smc/emcee.py:47-89).  Specification and counter layout: include/asmc.h (asmc_stretch_*), DESIGN.md §3.12.
//
// One Markov step is two half-sweeps.  In each, every walker k of the active half h picks a walker j uniformly from the other
// half (read as it stands after the previous half-sweep), draws zz = ((a - 1) u + 1)^2 / a, proposes y = x_j - (x_j - x_k) zz
// and accepts iff (d - 1) log zz + log p(y) - log p(x_k) > log u'.  The split is a counter-keyed bijection sigma of [0, n)
// (a Feistel network with cycle walking): walker i is in half sigma(i) & 1, the m-th member of half h is sigma^-1(2 m + h), so
// the halves hold exactly ceil(n / 2) and floor(n / 2) walkers without a scan or an index buffer.
//   k_stretch_propose  slot m of half h: gather x_k, x_j -> y[m, :] (compact [|half|, d]), logf[m] = (d - 1) log zz
//   (caller)           densities at y (transform inverse, flow log q, built-in mixtures or Python callables)
//   k_stretch_accept   tempered log-target of y and of x_k, accept, copy y[m] into row k and the new densities into the
//                      carried arrays; the accepts go to the step's device-resident counter.
// Writes touch only the active half's rows; the next half-sweep reads them in stream order: no grid barrier.
#include "asmc_pcn_dev.h"

#define STRETCH_TAG_DRAW 0x60000000u   // counter word 3 of the per-slot draws (| shard)
#define STRETCH_TAG_SPLIT 0xA0000000u  // counter word 3 of the split's Feistel round function (| shard)
#define STRETCH_ROUNDS 4
#define STRETCH_MAX_SHARD 0x10000000u

struct StretchArgs {
    int64_t n;        // walkers of the ensemble (this rank's shard)
    int64_t n_half;   // slots of the active half: (n + 1 - h) / 2
    int64_t n_other;  // walkers of the other half: (n + h) / 2
    uint32_t half;    // h
    uint32_t hbits;   // Feistel half width: ceil(ceil(log2 n) / 2)
    uint32_t step;    // counter word 1 of every draw of this step
    uint32_t shard;   // low bits of counter word 3 (this rank: each shard is its own ensemble)
    uint32_t k0, k1;  // Philox key: the mutation's seed
    double a;         // stretch scale
    int d, lg_tpr;    // row width; log2 of the lanes that share one row in the row passes
};

// ---- the split: Feistel network on 2 hbits bits, round function = word 0 of one Philox block ------------------------------
__device__ __forceinline__ uint32_t stretch_round(const StretchArgs& s, uint32_t r, uint32_t v) {
    uint32_t w[4];
    philox4x32_10(v, s.step, r, STRETCH_TAG_SPLIT | s.shard, s.k0, s.k1, w);
    return w[0] & ((1u << s.hbits) - 1u);
}

// sigma^-1: the inverse network, walked until the value falls inside [0, n) (cycle walking keeps it a bijection of [0, n))
__device__ __forceinline__ uint32_t stretch_sigma_inv(const StretchArgs& s, uint32_t v) {
    const uint32_t mask = (1u << s.hbits) - 1u;
    do {
        uint32_t L = v >> s.hbits, R = v & mask;
#pragma unroll
        for (int r = STRETCH_ROUNDS - 1; r >= 0; r--) {
            const uint32_t R0 = L;
            L = R ^ stretch_round(s, (uint32_t)r, L);
            R = R0;
        }
        v = (L << s.hbits) | R;
    } while ((int64_t)v >= s.n);
    return v;
}

// the per-slot draws of slot m: block b (0: the stretch variate u from words 0, 1 and the accept variate u' from words 2, 3;
// 1: the complementary slot m' = floor(w64 |other| / 2^64) from words 0 (high), 1 (low))
__device__ __forceinline__ void stretch_block(const StretchArgs& s, uint64_t m, uint32_t b, uint32_t w[4]) {
    philox4x32_10((uint32_t)m, s.step, (b << 1) | s.half, STRETCH_TAG_DRAW | s.shard, s.k0, s.k1, w);
}

__device__ __forceinline__ uint32_t stretch_walker(const StretchArgs& s, uint64_t m) {
    return stretch_sigma_inv(s, (uint32_t)(2 * m + s.half));
}

template <typename T>
__global__ __launch_bounds__(ASMC_BLOCK) void k_stretch_propose(const T* __restrict__ x, const StretchArgs s, T* __restrict__ y,
                                                                double* __restrict__ logf, unsigned long long* __restrict__ count) {
    __shared__ int64_t s_k[ASMC_BLOCK], s_j[ASMC_BLOCK];
    __shared__ double s_zz[ASMC_BLOCK];
    const int64_t m0 = (int64_t)blockIdx.x * ASMC_BLOCK;
    const int64_t m = m0 + threadIdx.x;
    if (count != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *count = 0;  // half 0 opens the step's counter
    if (m < s.n_half) {
        uint32_t w[4];
        stretch_block(s, (uint64_t)m, 0, w);
        const double u = u01_from_words(w[0], w[1]);
        stretch_block(s, (uint64_t)m, 1, w);
        const uint64_t hi = (uint64_t)w[0] * (uint64_t)s.n_other;
        const uint64_t lo = (uint64_t)w[1] * (uint64_t)s.n_other;
        const uint64_t mo = (hi + (lo >> 32)) >> 32;  // floor(((w0 << 32) | w1) |other| / 2^64), exact
        const double t1 = (s.a - 1.0) * u + 1.0;
        const double zz = t1 * t1 / s.a;
        s_k[threadIdx.x] = stretch_walker(s, (uint64_t)m);
        s_j[threadIdx.x] = stretch_sigma_inv(s, (uint32_t)(2 * mo + 1 - s.half));
        s_zz[threadIdx.x] = zz;
        logf[m] = (double)(s.d - 1) * log(zz);
    }
    __syncthreads();
    // row pass: 2^lg_tpr lanes per row, consecutive coordinates on consecutive lanes
    const int64_t rows = s.n_half - m0 < ASMC_BLOCK ? s.n_half - m0 : ASMC_BLOCK;
    const int tpr = 1 << s.lg_tpr;
    for (int64_t r = threadIdx.x >> s.lg_tpr; r < rows; r += ASMC_BLOCK >> s.lg_tpr) {
        const T* __restrict__ xk = x + s_k[r] * s.d;
        const T* __restrict__ xj = x + s_j[r] * s.d;
        T* __restrict__ yr = y + (m0 + r) * s.d;
        const double zz = s_zz[r];
        for (int c = threadIdx.x & (tpr - 1); c < s.d; c += tpr) {
            const double xjc = (double)xj[c];
            const double diff = xjc - (double)xk[c];
            yr[c] = (T)(xjc - diff * zz);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(ASMC_BLOCK) void k_stretch_accept(T* __restrict__ x, const StretchArgs s, const T* __restrict__ y,
                                                               const double* __restrict__ logf, double beta, double* __restrict__ ll,
                                                               double* __restrict__ lp, double* __restrict__ lq, double* __restrict__ lj,
                                                               const double* __restrict__ ll_new, const double* __restrict__ lp_new,
                                                               const double* __restrict__ lq_new, const double* __restrict__ lj_new,
                                                               unsigned long long* __restrict__ count) {
    __shared__ int64_t s_k[ASMC_BLOCK];  // the walker an accepted slot moves, -1: rejected
    const int64_t m0 = (int64_t)blockIdx.x * ASMC_BLOCK;
    const int64_t m = m0 + threadIdx.x;
    bool acc = false;
    if (m < s.n_half) {
        const int64_t k = stretch_walker(s, (uint64_t)m);
        uint32_t w[4];
        stretch_block(s, (uint64_t)m, 0, w);
        const double u = u01_from_words(w[2], w[3]);
        double nlp = log_p_t(ll_new[m], lp_new[m], lq_new[m], beta);
        double olp = log_p_t(ll[k], lp[k], lq[k], beta);
        if (lj != nullptr) {  // a chain in a preconditioned space: log|det dT^-1/dz| joins the log-target, NaN / +inf -> -inf again
            nlp = log_p_t_guard(nlp + lj_new[m]);
            olp = log_p_t_guard(olp + lj[k]);
        }
        const double lnpdiff = logf[m] + nlp - olp;  // emcee's order: (f + new) - old
        acc = lnpdiff > log(u);
        if (acc) {
            ll[k] = ll_new[m];
            lp[k] = lp_new[m];
            lq[k] = lq_new[m];
            if (lj != nullptr) lj[k] = lj_new[m];
        }
        s_k[threadIdx.x] = acc ? k : -1;
    }
    const unsigned long long ballot = __ballot(acc);
    if ((threadIdx.x & (ASMC_WAVE - 1)) == 0 && ballot != 0ull) atomicAdd(count, (unsigned long long)__popcll(ballot));
    __syncthreads();
    const int64_t rows = s.n_half - m0 < ASMC_BLOCK ? s.n_half - m0 : ASMC_BLOCK;
    const int tpr = 1 << s.lg_tpr;
    for (int64_t r = threadIdx.x >> s.lg_tpr; r < rows; r += ASMC_BLOCK >> s.lg_tpr) {
        const int64_t k = s_k[r];
        if (k < 0) continue;
        const T* __restrict__ yr = y + (m0 + r) * s.d;
        T* __restrict__ xr = x + k * s.d;
        for (int c = threadIdx.x & (tpr - 1); c < s.d; c += tpr) xr[c] = yr[c];
    }
}

static int stretch_args(asmc_ctx* ctx, int64_t n, int d, int x_dtype, int half, uint64_t seed, uint32_t shard, uint32_t step,
                        int t, StretchArgs& s) {
    ASMC_REQUIRE(ctx != nullptr, "null ctx");
    ASMC_REQUIRE(n >= 2 && n < (1LL << 31) && d > 0 && d <= ASMC_MAX_DIMS, "bad sizes (2 <= n < 2^31, 0 < d <= ASMC_MAX_DIMS)");
    ASMC_REQUIRE(x_dtype == ASMC_F64 || x_dtype == ASMC_F32, "bad x_dtype");
    ASMC_REQUIRE(half == 0 || half == 1, "half must be 0 or 1");
    ASMC_REQUIRE(shard < STRETCH_MAX_SHARD, "shard must be < 2^28");
    ASMC_REQUIRE(t >= 0 && t < ASMC_MAX_PCN_STEPS, "step index t out of range");
    memset(&s, 0, sizeof(s));
    s.n = n;
    s.half = (uint32_t)half;
    s.n_half = (n + 1 - half) / 2;
    s.n_other = (n + half) / 2;
    uint32_t bits = 0;
    while ((1LL << bits) < n) bits++;
    s.hbits = (bits + 1) / 2;
    s.step = step;
    s.shard = shard;
    s.k0 = (uint32_t)seed;
    s.k1 = (uint32_t)(seed >> 32);
    s.d = d;
    s.lg_tpr = 0;
    while ((1 << s.lg_tpr) < d && s.lg_tpr < 6) s.lg_tpr++;
    return ASMC_OK;
}

extern "C" {

int asmc_stretch_propose(asmc_ctx* ctx, int64_t n, int d, int x_dtype, const void* x, int half, double a, uint64_t seed,
                         uint32_t shard, uint32_t step, int t, void* y, double* logf, asmc_stream stream) {
    StretchArgs s;
    const int rc = stretch_args(ctx, n, d, x_dtype, half, seed, shard, step, t, s);
    if (rc) return rc;
    ASMC_REQUIRE(x && y && logf, "null pointer");
    ASMC_REQUIRE(a > 1.0 && a < INFINITY, "the stretch scale a must be finite and > 1");
    s.a = a;
    hipStream_t st = as_stream(stream);
    const int grid = (int)((s.n_half + ASMC_BLOCK - 1) / ASMC_BLOCK);
    unsigned long long* count = half == 0 ? ctx->d_stretch + t : nullptr;
    if (x_dtype == ASMC_F64)
        ASMC_LAUNCH(ctx, st, "k_stretch_propose", k_stretch_propose<double>, dim3(grid), dim3(ASMC_BLOCK), 0, st,
                    (const double*)x, s, (double*)y, logf, count);
    else
        ASMC_LAUNCH(ctx, st, "k_stretch_propose", k_stretch_propose<float>, dim3(grid), dim3(ASMC_BLOCK), 0, st,
                    (const float*)x, s, (float*)y, logf, count);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int asmc_stretch_accept(asmc_ctx* ctx, int64_t n, int d, int x_dtype, void* x, int half, const void* y,
                        const double* logf, double beta, double* ll, double* lp, double* lq, double* lj, const double* ll_new,
                        const double* lp_new, const double* lq_new, const double* lj_new, uint64_t seed, uint32_t shard,
                        uint32_t step, int t, asmc_stream stream) {
    StretchArgs s;
    const int rc = stretch_args(ctx, n, d, x_dtype, half, seed, shard, step, t, s);
    if (rc) return rc;
    ASMC_REQUIRE(x && y && logf && ll && lp && lq && ll_new && lp_new && lq_new, "null pointer");
    ASMC_REQUIRE((lj == nullptr) == (lj_new == nullptr), "log-Jacobian arrays: both or neither");
    hipStream_t st = as_stream(stream);
    const int grid = (int)((s.n_half + ASMC_BLOCK - 1) / ASMC_BLOCK);
    if (x_dtype == ASMC_F64)
        ASMC_LAUNCH(ctx, st, "k_stretch_accept", k_stretch_accept<double>, dim3(grid), dim3(ASMC_BLOCK), 0, st, (double*)x, s,
                    (const double*)y, logf, beta, ll, lp, lq, lj, ll_new, lp_new, lq_new, lj_new, ctx->d_stretch + t);
    else
        ASMC_LAUNCH(ctx, st, "k_stretch_accept", k_stretch_accept<float>, dim3(grid), dim3(ASMC_BLOCK), 0, st, (float*)x, s,
                    (const float*)y, logf, beta, ll, lp, lq, lj, ll_new, lp_new, lq_new, lj_new, ctx->d_stretch + t);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int asmc_stretch_counts(asmc_ctx* ctx, int n_steps, int64_t* counts_host, asmc_stream stream) {
    ASMC_REQUIRE(ctx && counts_host, "null pointer");
    ASMC_REQUIRE(n_steps >= 1 && n_steps <= ASMC_MAX_PCN_STEPS, "n_steps out of range");
    hipStream_t st = as_stream(stream);
    unsigned long long* h = reinterpret_cast<unsigned long long*>(ctx->h_pinned);
    ASMC_HIP(hipStreamSynchronize(st));  // pinned staging may still be in flight
    ASMC_HIP(hipMemcpyAsync(h, ctx->d_stretch, sizeof(unsigned long long) * n_steps, hipMemcpyDeviceToHost, st));
    ASMC_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < n_steps; i++) counts_host[i] = (int64_t)h[i];
    return ASMC_OK;
}

}  // extern "C"
