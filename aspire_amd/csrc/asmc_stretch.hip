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
#include "asmc_stretch_dev.h"

// the per-slot draws of slot m (stretch_block): block 0: the stretch variate u from words 0, 1 and the accept variate u' from
// words 2, 3; block 1: the complementary slot m' = floor(w64 |other| / 2^64) from words 0 (high), 1 (low)

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
        const uint64_t mo = stretch_index(w[0], w[1], (uint64_t)s.n_other);
        const double t1 = (s.a - 1.0) * u + 1.0;
        const double zz = t1 * t1 / s.a;
        s_k[threadIdx.x] = stretch_walker(s, (uint64_t)m);
        s_j[threadIdx.x] = stretch_member(s, mo, 1u - s.half);
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
    stretch_accept_body<T>(x, s, y, logf, beta, ll, lp, lq, lj, ll_new, lp_new, lq_new, lj_new, count);
}

extern "C" {

int asmc_stretch_propose(asmc_ctx* ctx, int64_t n, int d, int x_dtype, const void* x, int half, double a, uint64_t seed,
                         uint32_t shard, uint32_t step, int t, void* y, double* logf, asmc_stream stream) {
    StretchArgs s;
    const int rc = stretch_args(ctx, n, 2, d, x_dtype, 2, half, STRETCH_TAG_DRAW, seed, shard, step, t, s);
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
    const int rc = stretch_args(ctx, n, 2, d, x_dtype, 2, half, STRETCH_TAG_DRAW, seed, shard, step, t, s);
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
