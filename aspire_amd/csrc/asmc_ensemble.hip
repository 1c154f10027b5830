// asmc_ensemble.hip — the differential-evolution and snooker moves of the "emcee_smc" / "emcee" samplers: emcee's DEMove(sigma,
// gamma0) on a RedBlueMove with nsplits = 2 and DESnookerMove(gammas) with nsplits = 4, randomize_split = True (ter Braak 2006;
// ter Braak & Vrugt 2008).  Specification and counter layout: include/asmc.h (asmc_ensemble_*), DESIGN.md §3.26.
//
// One Markov step is S group-sweeps over the split of asmc_stretch_dev.h.  In each, every walker k of the active group draws its
// partners from the other groups (read as they stand after the previous sweep):
//   k_de_propose       slot m: two distinct walkers j1, j2 of the other half, gamma = g0 (1 + sigma xi),
//                      y[m, :] = x_k + gamma (x_j2 - x_j1), logf[m] = 0                                   (3 rows read, 1 written)
//   k_snooker_propose  slot m: one walker of each other group, shuffled into (z, z1, z2); the step along the line through z and
//                      x_k is gammas times the difference of the projections of z1 and z2 onto it,
//                      logf[m] = (d - 1) (log |y - z| - log |x_k - z|)                                    (4 rows read, 1 written)
//   (caller)           densities at y
//   k_ensemble_accept  the accept step of the stretch move (asmc_stretch_dev.h) on the S-way split
// Both proposal kernels follow k_stretch_propose: slot draws into LDS by one thread per slot, then 2^lg_tpr lanes per row.  The
// snooker's two row reductions pass over the coordinates once, the write of y a second time (the rows come from L2 then): no
// lane holds a row.
#include "asmc_stretch_dev.h"

template <typename T>
__global__ __launch_bounds__(ASMC_BLOCK) void k_de_propose(const T* __restrict__ x, const StretchArgs s, T* __restrict__ y,
                                                           double* __restrict__ logf, unsigned long long* __restrict__ count,
                                                           const double* __restrict__ bmtab) {
    __shared__ uint32_t s_k[ASMC_BLOCK], s_j1[ASMC_BLOCK], s_j2[ASMC_BLOCK];
    __shared__ double s_gamma[ASMC_BLOCK];
    bm_d2* bmt = bm_lds();
    bm_tab_stage<ASMC_BLOCK>(bmt, bmtab);
    __syncthreads();
    const int64_t m0 = (int64_t)blockIdx.x * ASMC_BLOCK;
    const int64_t m = m0 + threadIdx.x;
    if (count != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *count = 0;  // group 0 opens the step's counter
    if (m < s.n_half) {
        uint32_t w[4];
        stretch_block(s, (uint64_t)m, 0, w);
        const uint64_t m1 = stretch_index(w[0], w[1], (uint64_t)s.n_other);
        stretch_block(s, (uint64_t)m, 1, w);
        uint64_t m2 = stretch_index(w[0], w[1], (uint64_t)s.n_other - 1);
        m2 += m2 >= m1 ? 1 : 0;
        double xi, xi_odd;
        bm_pair32(w[2], w[3], bmt, xi, xi_odd);
        s_k[threadIdx.x] = stretch_walker(s, (uint64_t)m);
        s_j1[threadIdx.x] = stretch_member(s, m1, 1u - s.half);
        s_j2[threadIdx.x] = stretch_member(s, m2, 1u - s.half);
        s_gamma[threadIdx.x] = s.a * (1.0 + s.b * xi);
        logf[m] = 0.0;
    }
    __syncthreads();
    const int64_t rows = s.n_half - m0 < ASMC_BLOCK ? s.n_half - m0 : ASMC_BLOCK;
    const int tpr = 1 << s.lg_tpr;
    for (int64_t r = threadIdx.x >> s.lg_tpr; r < rows; r += ASMC_BLOCK >> s.lg_tpr) {
        const T* __restrict__ xk = x + (int64_t)s_k[r] * s.d;
        const T* __restrict__ x1 = x + (int64_t)s_j1[r] * s.d;
        const T* __restrict__ x2 = x + (int64_t)s_j2[r] * s.d;
        T* __restrict__ yr = y + (m0 + r) * s.d;
        const double gamma = s_gamma[r];
        for (int c = threadIdx.x & (tpr - 1); c < s.d; c += tpr) {
            const double diff = (double)x2[c] - (double)x1[c];
            yr[c] = (T)((double)xk[c] + gamma * diff);
        }
    }
}

// sum over the 2^lg lanes that share a row: a butterfly, every lane of the row ends with the same bits (hmc_row_sum with lg at run time)
__device__ __forceinline__ double ensemble_row_sum(double v, int lg) {
    for (int o = (1 << lg) >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <typename T>
__global__ __launch_bounds__(ASMC_BLOCK) void k_snooker_propose(const T* __restrict__ x, const StretchArgs s, T* __restrict__ y,
                                                                double* __restrict__ logf, unsigned long long* __restrict__ count) {
    __shared__ uint32_t s_k[ASMC_BLOCK], s_z[ASMC_BLOCK], s_z1[ASMC_BLOCK], s_z2[ASMC_BLOCK];
    const int64_t m0 = (int64_t)blockIdx.x * ASMC_BLOCK;
    const int64_t m = m0 + threadIdx.x;
    if (count != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *count = 0;  // group 0 opens the step's counter
    if (m < s.n_half) {
        const uint32_t g = s.half;
        const uint32_t o0 = g > 0 ? 0u : 1u, o1 = g > 1 ? 1u : 2u, o2 = g > 2 ? 2u : 3u;  // the other groups, ascending
        uint32_t w[4], c[3];
        stretch_block(s, (uint64_t)m, 0, w);
        c[0] = stretch_member(s, stretch_index(w[0], w[1], (uint64_t)((s.n - o0 + 3) >> 2)), o0);
        stretch_block(s, (uint64_t)m, 1, w);
        c[1] = stretch_member(s, stretch_index(w[0], w[1], (uint64_t)((s.n - o1 + 3) >> 2)), o1);
        c[2] = stretch_member(s, stretch_index(w[2], w[3], (uint64_t)((s.n - o2 + 3) >> 2)), o2);
        stretch_block(s, (uint64_t)m, 2, w);
        const uint32_t r = (uint32_t)(((uint64_t)w[0] * 6ull) >> 32);
        // the r-th permutation of (0, 1, 2) in lexicographic order
        const uint32_t p0 = r >> 1;
        const uint32_t lo = p0 == 0 ? 1u : 0u, hi = p0 == 2 ? 1u : 2u;  // the two that remain, ascending
        const uint32_t p1 = (r & 1u) ? hi : lo, p2 = (r & 1u) ? lo : hi;
        s_k[threadIdx.x] = stretch_walker(s, (uint64_t)m);
        s_z[threadIdx.x] = p0 == 0 ? c[0] : p0 == 1 ? c[1] : c[2];
        s_z1[threadIdx.x] = p1 == 0 ? c[0] : p1 == 1 ? c[1] : c[2];
        s_z2[threadIdx.x] = p2 == 0 ? c[0] : p2 == 1 ? c[1] : c[2];
    }
    __syncthreads();
    const int64_t rows = s.n_half - m0 < ASMC_BLOCK ? s.n_half - m0 : ASMC_BLOCK;
    const int tpr = 1 << s.lg_tpr;
    const int lane = threadIdx.x & (tpr - 1);
    // (the lanes of a row share r, so they run the same trips and meet in the butterflies)
    for (int64_t r = threadIdx.x >> s.lg_tpr; r < rows; r += ASMC_BLOCK >> s.lg_tpr) {
        const T* __restrict__ xk = x + (int64_t)s_k[r] * s.d;
        const T* __restrict__ xz = x + (int64_t)s_z[r] * s.d;
        const T* __restrict__ x1 = x + (int64_t)s_z1[r] * s.d;
        const T* __restrict__ x2 = x + (int64_t)s_z2[r] * s.d;
        T* __restrict__ yr = y + (m0 + r) * s.d;
        double ss = 0.0, dp = 0.0;
        for (int c = lane; c < s.d; c += tpr) {
            const double delta = (double)xk[c] - (double)xz[c];
            ss += delta * delta;
            dp += delta * ((double)x1[c] - (double)x2[c]);
        }
        ss = ensemble_row_sum(ss, s.lg_tpr);
        dp = ensemble_row_sum(dp, s.lg_tpr);
        const double r0 = sqrt(ss);
        const bool ok = r0 > 0.0 && r0 < INFINITY;
        const double proj = dp / r0;
        const double gp = s.a * proj;
        if (ok) {
            for (int c = lane; c < s.d; c += tpr) {
                const double xkc = (double)xk[c];
                const double delta = xkc - (double)xz[c];
                yr[c] = (T)(xkc + gp * (delta / r0));
            }
        } else {
            for (int c = lane; c < s.d; c += tpr) yr[c] = xk[c];
        }
        if (lane == 0) {
            const double r1 = fabs(r0 + gp);
            logf[m0 + r] = (ok && r1 > 0.0 && r1 < INFINITY) ? (double)(s.d - 1) * (log(r1) - log(r0)) : -INFINITY;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(ASMC_BLOCK) void k_ensemble_accept(T* __restrict__ x, const StretchArgs s, const T* __restrict__ y,
                                                                const double* __restrict__ logf, double beta, double* __restrict__ ll,
                                                                double* __restrict__ lp, double* __restrict__ lq, double* __restrict__ lj,
                                                                const double* __restrict__ ll_new, const double* __restrict__ lp_new,
                                                                const double* __restrict__ lq_new, const double* __restrict__ lj_new,
                                                                unsigned long long* __restrict__ count) {
    stretch_accept_body<T>(x, s, y, logf, beta, ll, lp, lq, lj, ll_new, lp_new, lq_new, lj_new, count);
}

extern "C" {

int asmc_ensemble_propose(asmc_ctx* ctx, int64_t n, int d, int x_dtype, const void* x, int move, int nsplits, int group, double p0,
                          double p1, uint64_t seed, uint32_t shard, uint32_t step, int t, void* y, double* logf,
                          asmc_stream stream) {
    ASMC_REQUIRE(move == ASMC_MOVE_DE || move == ASMC_MOVE_SNOOKER, "move must be ASMC_MOVE_DE or ASMC_MOVE_SNOOKER");
    ASMC_REQUIRE(nsplits == (move == ASMC_MOVE_DE ? 2 : 4), "nsplits must be 2 for the DE move and 4 for the snooker move");
    StretchArgs s;
    const int rc = stretch_args(ctx, n, 4, d, x_dtype, nsplits, group, ENSEMBLE_TAG_DRAW, seed, shard, step, t, s);
    if (rc) return rc;
    ASMC_REQUIRE(x && y && logf, "null pointer");
    ASMC_REQUIRE(fabs(p0) < INFINITY, move == ASMC_MOVE_DE ? "the DE scale g0 must be finite" : "the snooker scale gammas must be finite");
    ASMC_REQUIRE(move != ASMC_MOVE_DE || fabs(p1) < INFINITY, "the DE spread sigma must be finite");
    s.a = p0;
    s.b = p1;
    hipStream_t st = as_stream(stream);
    const int grid = (int)((s.n_half + ASMC_BLOCK - 1) / ASMC_BLOCK);
    unsigned long long* count = group == 0 ? ctx->d_stretch + t : nullptr;
    if (move == ASMC_MOVE_DE) {
        if (x_dtype == ASMC_F64)
            ASMC_LAUNCH(ctx, st, "k_de_propose", k_de_propose<double>, dim3(grid), dim3(ASMC_BLOCK), 0, st, (const double*)x, s,
                        (double*)y, logf, count, (const double*)ctx->d_bmtab);
        else
            ASMC_LAUNCH(ctx, st, "k_de_propose", k_de_propose<float>, dim3(grid), dim3(ASMC_BLOCK), 0, st, (const float*)x, s,
                        (float*)y, logf, count, (const double*)ctx->d_bmtab);
    } else {
        if (x_dtype == ASMC_F64)
            ASMC_LAUNCH(ctx, st, "k_snooker_propose", k_snooker_propose<double>, dim3(grid), dim3(ASMC_BLOCK), 0, st,
                        (const double*)x, s, (double*)y, logf, count);
        else
            ASMC_LAUNCH(ctx, st, "k_snooker_propose", k_snooker_propose<float>, dim3(grid), dim3(ASMC_BLOCK), 0, st,
                        (const float*)x, s, (float*)y, logf, count);
    }
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int asmc_ensemble_accept(asmc_ctx* ctx, int64_t n, int d, int x_dtype, void* x, int nsplits, int group, const void* y,
                         const double* logf, double beta, double* ll, double* lp, double* lq, double* lj, const double* ll_new,
                         const double* lp_new, const double* lq_new, const double* lj_new, uint64_t seed, uint32_t shard,
                         uint32_t step, int t, asmc_stream stream) {
    StretchArgs s;
    const int rc = stretch_args(ctx, n, 4, d, x_dtype, nsplits, group, ENSEMBLE_TAG_DRAW, seed, shard, step, t, s);
    if (rc) return rc;
    ASMC_REQUIRE(x && y && logf && ll && lp && lq && ll_new && lp_new && lq_new, "null pointer");
    ASMC_REQUIRE((lj == nullptr) == (lj_new == nullptr), "log-Jacobian arrays: both or neither");
    hipStream_t st = as_stream(stream);
    const int grid = (int)((s.n_half + ASMC_BLOCK - 1) / ASMC_BLOCK);
    if (x_dtype == ASMC_F64)
        ASMC_LAUNCH(ctx, st, "k_ensemble_accept", k_ensemble_accept<double>, dim3(grid), dim3(ASMC_BLOCK), 0, st, (double*)x, s,
                    (const double*)y, logf, beta, ll, lp, lq, lj, ll_new, lp_new, lq_new, lj_new, ctx->d_stretch + t);
    else
        ASMC_LAUNCH(ctx, st, "k_ensemble_accept", k_ensemble_accept<float>, dim3(grid), dim3(ASMC_BLOCK), 0, st, (float*)x, s,
                    (const float*)y, logf, beta, ll, lp, lq, lj, ll_new, lp_new, lq_new, lj_new, ctx->d_stretch + t);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

}  // extern "C"
