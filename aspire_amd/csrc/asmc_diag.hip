// asmc_diag.hip - diagnostics of a recorded chain, reduced where the chain lies (include/asmc.h, ABI 31):
// emcee's integrated autocorrelation time, lag for lag, and split R-hat.
//
// A chain is [S, W, pitch] of fp32 or fp64, element (t, w, j) at t W pitch + w pitch + j: the layout of asmc_chain_target from its
// first kept step on.  A series is one coordinate of one walker over the S steps.  A lane owns a series; at fixed t the lanes of a
// wave read consecutive elements (pitch == d), so every load is coalesced.  All arithmetic is fp64 whatever the chain's type, every
// index is 64-bit, nothing outside the S kept steps is read.  No floating-point atomics: sums across walkers go lane -> block
// partial (LDS, walker order) -> finishing kernel (block order), the same order in every run.
#include "asmc_common.h"

#define DIAG_BLOCK 256
#define DIAG_MAX_PITCH (1 << 20)  // a lane's offset within a block's rows stays a 32-bit number
// grids in whole rounds of what is resident at once (every block of a launch does the same work, so a part-filled last round is lost time)
#define DIAG_ACF_GRID 2048  // lag-block kernel: 256 CUs x 2 resident blocks x 4 rounds (KB = 32: 225 VGPRs, 64 KB LDS), x 4 x 2 (KB = 16: 118, 32 KB)
#define DIAG_MOM_GRID 1792  // moments kernel: 256 CUs x 7 resident blocks (72 VGPRs)

// ---- per-series mean and centred sum of squares -----------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void series_moments(const T* __restrict__ p, int64_t step, int64_t t0, int64_t n, double* mean_out,
                                               double* c0_out) {
    const T* q = p + t0 * step;
    double s = 0.0;
#pragma unroll 8
    for (int64_t t = 0; t < n; ++t) s += (double)q[t * step];
    const double m = s / (double)n;  // (n = 0: NaN)
    double c = 0.0;
#pragma unroll 8
    for (int64_t t = 0; t < n; ++t) {
        const double dv = (double)q[t * step] - m;
        c = fma(dv, dv, c);
    }
    *mean_out = m;
    *c0_out = c;
}

template <typename T>
__global__ __launch_bounds__(DIAG_BLOCK) void k_chain_moments(const T* __restrict__ x, int64_t S, int64_t W, int d, int64_t pitch,
                                                              int halves, double* __restrict__ mean, double* __restrict__ c0) {
    const int64_t n = W * d, step = W * pitch;
    const int64_t stride = (int64_t)gridDim.x * DIAG_BLOCK;
    for (int64_t e = (int64_t)blockIdx.x * DIAG_BLOCK + threadIdx.x; e < n; e += stride) {
        const int64_t w = e / d;
        const T* p = x + w * pitch + (e - w * d);
        if (!halves) {
            series_moments(p, step, 0, S, mean + e, c0 + e);
        } else {  // the first and the last S / 2 steps (an odd S drops its middle step)
            const int64_t h = S / 2;
            series_moments(p, step, 0, h, mean + e, c0 + e);
            series_moments(p, step, S - h, h, mean + n + e, c0 + n + e);
        }
    }
}

// ---- one block of KB lags ---------------------------------------------------------------------------------------------------
// Per series y_t = x_t - mean, zero beyond the chain's end: acc[kk] = sum_t y_t y_{t + k0 + kk}.  The sweep advances KB steps at a
// time with KB leading values (lead), the 2 KB trailing values they meet (cur | nxt) and the KB sums in registers; the KB x KB
// products of a chunk are unrolled, so every register index is a constant.  A block covers wpb whole walkers x all d coordinates -
// lane l is walker l / d, coordinate l % d of its group, series (g wpb d + l): consecutive lanes, consecutive addresses - and walks
// the groups g = blockIdx, blockIdx + grid, ...; the lane's LDS cells collect acc / c0 over its groups in that order.
template <typename T, int KB>
__global__ __launch_bounds__(DIAG_BLOCK) void k_chain_acf_block(const T* __restrict__ x, int64_t S, int64_t W, int d, int64_t pitch,
                                                                int64_t k0, int wpb, const double* __restrict__ mean,
                                                                const double* __restrict__ c0, double* __restrict__ part) {
    __shared__ double sh[KB * DIAG_BLOCK];
    const int lane = threadIdx.x;
    const int used = wpb * d;
    const int wl = lane / d, j = lane - wl * d;
    const int64_t step = W * pitch;
    const int64_t groups = (W + wpb - 1) / wpb;
#pragma unroll
    for (int i = 0; i < KB; ++i) sh[i * DIAG_BLOCK + lane] = 0.0;  // the lane's own cells: its sums over its groups (idle lanes: 0)
    const unsigned lo = (unsigned)(wl * (int)pitch + j);  // the lane's element within its group's rows (pitch <= 2^20)
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t w = g * wpb + wl;
        if (lane >= used || w >= W) continue;
        const int64_t c = w * d + j;
        const double m = mean[c];
        const T* xg = x + g * wpb * pitch;  // uniform: a load is a scalar base plus the lane's 32-bit offset
        // a step beyond the chain's end is 0: the load goes to the last kept step instead and a select drops it - no branch sits
        // between the loads of a chunk, which all fly at once
        auto at = [&](int64_t t) {
            const double v = (double)(xg + (t < S ? t : S - 1) * step)[lo] - m;
            return t < S ? v : 0.0;
        };
        double acc[KB], lead[KB], cur[KB], nxt[KB];
#pragma unroll
        for (int i = 0; i < KB; ++i) {
            acc[i] = 0.0;
            cur[i] = at(k0 + i);
        }
        for (int64_t t0 = 0; t0 + k0 < S; t0 += KB) {
#pragma unroll
            for (int i = 0; i < KB; ++i) {
                lead[i] = at(t0 + i);
                nxt[i] = at(t0 + k0 + KB + i);
            }
#pragma unroll
            for (int i = 0; i < KB; ++i)
#pragma unroll
                for (int kk = 0; kk < KB; ++kk) acc[kk] = fma(lead[i], i + kk < KB ? cur[i + kk] : nxt[i + kk - KB], acc[kk]);
#pragma unroll
            for (int i = 0; i < KB; ++i) cur[i] = nxt[i];
        }
        const double v = c0[c];
#pragma unroll
        for (int i = 0; i < KB; ++i) sh[i * DIAG_BLOCK + lane] += acc[i] / v;  // (a series that never moves: 0 / 0 = NaN, as in emcee)
    }
    __syncthreads();
    for (int o = lane; o < d * KB; o += DIAG_BLOCK) {
        const int kk = o / d, jj = o - kk * d;
        double s = 0.0;
        for (int q = 0; q < wpb; ++q) s += sh[kk * DIAG_BLOCK + q * d + jj];
        part[((int64_t)blockIdx.x * d + jj) * KB + kk] = s;
    }
}

// ---- block partials -> rho of the block's lags -> the window's state ---------------------------------------------------------------
// state [4, d]: running sum of rho | done (0 / 1) | window | tau.  Block j: thread (q, kk) adds the partials of blocks q, q + nq, ...
// for lag kk, a tree over q, then thread 0 walks the lags in order.
__global__ __launch_bounds__(DIAG_BLOCK) void k_chain_acf_finish(const double* __restrict__ part, int nblocks, int d, int kb, int64_t k0,
                                                                 int64_t S, int64_t W, double c, double* __restrict__ state,
                                                                 double* __restrict__ rho_out, int64_t rho_pitch) {
    __shared__ double sh[DIAG_BLOCK];
    const int j = blockIdx.x, tid = threadIdx.x;
    const int kk = tid % kb, q = tid / kb, nq = DIAG_BLOCK / kb;
    double s = 0.0;
    for (int b = q; b < nblocks; b += nq) s += part[((int64_t)b * d + j) * kb + kk];
    sh[tid] = s;
    __syncthreads();
    for (int o = nq / 2; o > 0; o >>= 1) {
        if (q < o) sh[tid] += sh[tid + o * kb];
        __syncthreads();
    }
    if (tid != 0) return;
    double run = k0 == 0 ? 0.0 : state[j];
    bool done = k0 == 0 ? false : state[d + j] != 0.0;
    if (done) return;
    for (int i = 0; i < kb; ++i) {
        const int64_t k = k0 + i;
        if (k >= S) break;
        const double rho = sh[i] / (double)W;
        if (rho_out != nullptr) rho_out[(int64_t)j * rho_pitch + k] = rho;
        run += rho;
        const double tau = 2.0 * run - 1.0;
        if (!((double)k < c * tau) || k == S - 1) {  // Sokal's window: the first lag with k >= c tau_k; NaN: no window, the last lag
            done = true;
            state[2 * d + j] = (double)(tau != tau ? S - 1 : k);
            state[3 * d + j] = tau;
            break;
        }
    }
    state[j] = run;
    state[d + j] = done ? 1.0 : 0.0;
}

// ---- split R-hat from the half-series moments -------------------------------------------------------------------------------
// The m = 2 W half-chains are the rows of hmean / hc0 [m, d].  Two stages - the grand mean, then the squared deviations from it and
// the variances -, each a partial kernel and a finishing kernel.  Partial kernel: thread (r, j) of block b adds coordinate j of the
// rows b rpb + r, b rpb + r + grid rpb, ... (rpb = 256 / d whole rows per block and turn: consecutive threads, consecutive
// addresses), the rpb row-threads of a coordinate are added in order -> part [grid, 2, d].  Finishing kernel: thread j adds the
// blocks' partials in block order.
#define DIAG_RHAT_BLOCKS 240  // (240 x 2 x 256 + 256 doubles fit the context's block-partial scratch)

template <int STAGE>
__global__ __launch_bounds__(DIAG_BLOCK) void k_chain_rhat_part(const double* __restrict__ hmean, const double* __restrict__ hc0, int64_t M,
                                                                int d, const double* __restrict__ grand, double* __restrict__ part) {
    __shared__ double sh[2 * DIAG_BLOCK];
    const int rpb = DIAG_BLOCK / d, tid = threadIdx.x, r = tid / d, j = tid - r * d;
    double a = 0.0, b = 0.0;
    if (r < rpb) {
        const double g = STAGE ? grand[j] : 0.0;
        for (int64_t ci = (int64_t)blockIdx.x * rpb + r; ci < M; ci += (int64_t)gridDim.x * rpb) {
            if (STAGE == 0) {
                a += hmean[ci * d + j];
            } else {
                const double dv = hmean[ci * d + j] - g;
                a = fma(dv, dv, a);
                b += hc0[ci * d + j];
            }
        }
    }
    sh[tid] = a;
    sh[DIAG_BLOCK + tid] = b;
    __syncthreads();
    if (tid < d) {
        double s = 0.0, s2 = 0.0;
        for (int q = 0; q < rpb; ++q) {
            s += sh[q * d + tid];
            s2 += sh[DIAG_BLOCK + q * d + tid];
        }
        part[((int64_t)blockIdx.x * 2 + 0) * d + tid] = s;
        part[((int64_t)blockIdx.x * 2 + 1) * d + tid] = s2;
    }
}

// one block; STAGE 0: grand[j] <- the mean of the half-chains' means; STAGE 1: out[j] <- R-hat (n: the half-chains' length)
template <int STAGE>
__global__ __launch_bounds__(DIAG_BLOCK) void k_chain_rhat_finish(const double* __restrict__ part, int nblocks, int64_t M, int d, int64_t n,
                                                                  double* __restrict__ grand, double* __restrict__ out) {
    const int j = threadIdx.x;
    if (j >= d) return;
    double s = 0.0, s2 = 0.0;
    for (int b = 0; b < nblocks; ++b) {
        s += part[((int64_t)b * 2 + 0) * d + j];
        s2 += part[((int64_t)b * 2 + 1) * d + j];
    }
    if (STAGE == 0) {
        grand[j] = s / (double)M;
        return;
    }
    if (n < 2) {
        out[j] = __longlong_as_double(0x7ff8000000000000LL);
        return;
    }
    const double nn = (double)n;
    const double B = nn / (double)(M - 1) * s;
    const double Wv = s2 / (nn - 1.0) / (double)M;
    out[j] = sqrt(((nn - 1.0) / nn * Wv + B / nn) / Wv);
}

static int diag_check(const char* who, const asmc_ctx* ctx, int x_dtype, const void* x, int64_t S, int64_t W, int d, int64_t pitch) {
    if (ctx == nullptr || x == nullptr) {
        asmc_set_error("%s: null pointer", who);
        return ASMC_ERR_ARG;
    }
    if (x_dtype != ASMC_F64 && x_dtype != ASMC_F32) {
        asmc_set_error("%s: bad x_dtype", who);
        return ASMC_ERR_ARG;
    }
    if (S < 1 || W < 1 || d < 1 || d > ASMC_MAX_DIMS || pitch < d || pitch > DIAG_MAX_PITCH) {
        asmc_set_error("%s: bad sizes (S >= 1, W >= 1, 1 <= d <= %d, d <= pitch <= 2^20)", who, ASMC_MAX_DIMS);
        return ASMC_ERR_ARG;
    }
    return ASMC_OK;
}

static inline int diag_wpb(int d) { return DIAG_BLOCK / d; }  // whole walkers per block (d <= 256: at least one)

extern "C" {

int asmc_chain_acf_kb(void) { return ASMC_DIAG_KB; }

int asmc_chain_acf_blocks(int64_t n_walkers, int d) {
    if (n_walkers < 1 || d < 1 || d > ASMC_MAX_DIMS) return 0;
    const int wpb = diag_wpb(d);
    return grid_for((n_walkers + wpb - 1) / wpb, 1, DIAG_ACF_GRID);
}

int asmc_chain_series_moments(asmc_ctx* ctx, int x_dtype, const void* x_dev, int64_t n_steps, int64_t n_walkers, int d, int64_t pitch,
                              int halves, double* mean_dev, double* c0_dev, asmc_stream stream) {
    int rc = diag_check(__func__, ctx, x_dtype, x_dev, n_steps, n_walkers, d, pitch);
    if (rc) return rc;
    ASMC_REQUIRE(mean_dev != nullptr && c0_dev != nullptr, "null output");
    ASMC_REQUIRE(halves == 0 || halves == 1, "halves is 0 or 1");
    hipStream_t st = as_stream(stream);
    const int grid = grid_for(n_walkers * d, DIAG_BLOCK, DIAG_MOM_GRID);
    if (x_dtype == ASMC_F64)
        ASMC_LAUNCH(ctx, st, "k_chain_moments", k_chain_moments<double>, dim3(grid), dim3(DIAG_BLOCK), 0, st, (const double*)x_dev,
                    n_steps, n_walkers, d, pitch, halves, mean_dev, c0_dev);
    else
        ASMC_LAUNCH(ctx, st, "k_chain_moments", k_chain_moments<float>, dim3(grid), dim3(DIAG_BLOCK), 0, st, (const float*)x_dev,
                    n_steps, n_walkers, d, pitch, halves, mean_dev, c0_dev);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int asmc_chain_acf_block(asmc_ctx* ctx, int x_dtype, const void* x_dev, int64_t n_steps, int64_t n_walkers, int d, int64_t pitch,
                         int64_t k0, int kb, const double* mean_dev, const double* c0_dev, double* partials_dev, asmc_stream stream) {
    int rc = diag_check(__func__, ctx, x_dtype, x_dev, n_steps, n_walkers, d, pitch);
    if (rc) return rc;
    ASMC_REQUIRE(mean_dev != nullptr && c0_dev != nullptr && partials_dev != nullptr, "null moments / partials");
    ASMC_REQUIRE(kb == 16 || kb == 32, "kb is 16 or 32");
    ASMC_REQUIRE(k0 >= 0 && k0 % kb == 0, "k0 is a non-negative multiple of kb");
    hipStream_t st = as_stream(stream);
    const int wpb = diag_wpb(d);
    const int grid = asmc_chain_acf_blocks(n_walkers, d);
#define DIAG_ACF(T, KB)                                                                                                              \
    ASMC_LAUNCH(ctx, st, "k_chain_acf_block", (k_chain_acf_block<T, KB>), dim3(grid), dim3(DIAG_BLOCK), 0, st, (const T*)x_dev, n_steps, \
                n_walkers, d, pitch, k0, wpb, mean_dev, c0_dev, partials_dev)
    if (x_dtype == ASMC_F64 && kb == 16)
        DIAG_ACF(double, 16);
    else if (x_dtype == ASMC_F64)
        DIAG_ACF(double, 32);
    else if (kb == 16)
        DIAG_ACF(float, 16);
    else
        DIAG_ACF(float, 32);
#undef DIAG_ACF
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int asmc_chain_acf_finish(asmc_ctx* ctx, int64_t n_steps, int64_t n_walkers, int d, int64_t k0, int kb, double c,
                          const double* partials_dev, double* state_dev, double* rho_dev, int64_t rho_pitch, asmc_stream stream) {
    ASMC_REQUIRE(ctx != nullptr && partials_dev != nullptr && state_dev != nullptr, "null pointer");
    ASMC_REQUIRE(n_steps >= 1 && n_walkers >= 1 && d >= 1 && d <= ASMC_MAX_DIMS, "bad sizes");
    ASMC_REQUIRE(kb == 16 || kb == 32, "kb is 16 or 32");
    ASMC_REQUIRE(k0 >= 0 && k0 % kb == 0, "k0 is a non-negative multiple of kb");
    ASMC_REQUIRE(rho_dev == nullptr || rho_pitch >= n_steps, "rho rows shorter than the chain");
    hipStream_t st = as_stream(stream);
    ASMC_LAUNCH(ctx, st, "k_chain_acf_finish", k_chain_acf_finish, dim3(d), dim3(DIAG_BLOCK), 0, st, partials_dev,
                asmc_chain_acf_blocks(n_walkers, d), d, kb, k0, n_steps, n_walkers, c, state_dev, rho_dev, rho_pitch);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int asmc_chain_rhat(asmc_ctx* ctx, int64_t n_steps, int64_t n_walkers, int d, const double* half_mean_dev, const double* half_c0_dev,
                    double* rhat_dev, asmc_stream stream) {
    ASMC_REQUIRE(ctx != nullptr && half_mean_dev != nullptr && half_c0_dev != nullptr && rhat_dev != nullptr, "null pointer");
    ASMC_REQUIRE(n_steps >= 1 && n_walkers >= 1 && d >= 1 && d <= ASMC_MAX_DIMS, "bad sizes");
    hipStream_t st = as_stream(stream);
    const int64_t M = 2 * n_walkers;
    const int rpb = DIAG_BLOCK / d;
    const int grid = grid_for((M + rpb - 1) / rpb, 1, DIAG_RHAT_BLOCKS);
    double* part = ctx->d_partials;  // [grid, 2, d] | grand [d]: inside ASMC_MAX_BLOCKS * ASMC_MAX_BETAS * 2 doubles
    double* grand = part + (size_t)DIAG_RHAT_BLOCKS * 2 * ASMC_MAX_DIMS;
    static_assert((size_t)DIAG_RHAT_BLOCKS * 2 * ASMC_MAX_DIMS + ASMC_MAX_DIMS <= (size_t)ASMC_MAX_BLOCKS * ASMC_MAX_BETAS * 2,
                  "R-hat's partials outgrow the context's scratch");
    ASMC_LAUNCH(ctx, st, "k_chain_rhat_part", k_chain_rhat_part<0>, dim3(grid), dim3(DIAG_BLOCK), 0, st, half_mean_dev, half_c0_dev, M, d,
                (const double*)nullptr, part);
    ASMC_LAUNCH(ctx, st, "k_chain_rhat", k_chain_rhat_finish<0>, dim3(1), dim3(DIAG_BLOCK), 0, st, (const double*)part, grid, M, d,
                n_steps / 2, grand, rhat_dev);
    ASMC_LAUNCH(ctx, st, "k_chain_rhat_part", k_chain_rhat_part<1>, dim3(grid), dim3(DIAG_BLOCK), 0, st, half_mean_dev, half_c0_dev, M, d,
                (const double*)grand, part);
    ASMC_LAUNCH(ctx, st, "k_chain_rhat", k_chain_rhat_finish<1>, dim3(1), dim3(DIAG_BLOCK), 0, st, (const double*)part, grid, M, d,
                n_steps / 2, grand, rhat_dev);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

}  // extern "C"
