// asmc_density.hip — analytic Gaussian proposal draw and the built-in diagonal-mixture log-density.
//
// Replaces (reference mj-will/aspire):
//   src/aspire/samplers/mcmc.py:66-67  flow.sample_and_log_prob for the analytic Gaussian proposal
#include <stdlib.h>

#include "asmc_pcn_shared.h"
#include "asmc_transform_dev.h"  // clip

// =============================================================================================
// analytic Gaussian proposal draw, built-in density evaluation
// =============================================================================================
template <typename T>
__global__ __launch_bounds__(ASMC_BLOCK) void k_gaussian_draw(int64_t n, int d, const double* __restrict__ mu,
                                                             const double* __restrict__ sigma,
                                                             unsigned long long seed, unsigned long long gid0,
                                                             uint32_t draw_id, T* __restrict__ x,
                                                             const double* __restrict__ bmtab) {
    bm_d2* bmt = bm_lds();
    bm_tab_stage<ASMC_BLOCK>(bmt, bmtab);
    __syncthreads();
    const int quads = (d + 3) / 4;  // one Philox block = four coordinates (asmc_pcn_dev.h normal_quad)
    const int64_t total = n * quads;
    const int64_t stride = (int64_t)gridDim.x * ASMC_BLOCK;
    for (int64_t e = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x; e < total; e += stride) {
        const int64_t i = e / quads;
        const int qd = (int)(e - i * quads);
        double z[4];
        normal_quad(seed, gid0 + (unsigned long long)i, draw_id, (uint32_t)qd, bmt, z[0], z[1], z[2], z[3]);
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int j = 4 * qd + c;
            if (j < d) x[i * d + j] = (T)fma(sigma[j], z[c], mu[j]);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(ASMC_BLOCK) void k_gaussian_logq(int64_t n, int d, const double* __restrict__ mu,
                                                             const double* __restrict__ sigma,
                                                             const T* __restrict__ x, double* __restrict__ lq) {
    const int64_t stride = (int64_t)gridDim.x * ASMC_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x; i < n; i += stride) {
        double q = 0.0, ls = 0.0;
        for (int j = 0; j < d; j++) {
            const double z = ((double)x[i * d + j] - mu[j]) / sigma[j];
            q = fma(z, z, q);
            ls += log(sigma[j]);
        }
        lq[i] = -0.5 * q - ls - 0.5 * (double)d * 1.8378770664093454835606594728112;  // log(2 pi)
    }
}

template <typename T, int VEC>
__global__ __launch_bounds__(ASMC_BLOCK) void k_mixture_logpdf(int64_t n, int d, const T* __restrict__ x,
                                                              MixDev m, double* __restrict__ out,
                                                              int waves_per_block) {
    extern __shared__ __align__(16) char smem[];
    const int rowbytes = d * (int)sizeof(T);
    const int ldsrow = lds_row_stride(rowbytes);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    char* tile = smem + (size_t)wave * 64 * ldsrow;
    const int64_t n_tiles = (n + 63) / 64;
    for (int64_t tile0 = (int64_t)blockIdx.x * waves_per_block; tile0 < n_tiles;
         tile0 += (int64_t)gridDim.x * waves_per_block) {
        const int64_t t = tile0 + wave;
        const bool active = t < n_tiles;
        const int64_t i = t * 64 + lane;
        const int64_t row0 = t * 64;
        const int64_t valid_bytes = active ? (((n - row0) < 64 ? (n - row0) : 64) * (int64_t)rowbytes) : 0;
        if (active) tile_load<VEC>(reinterpret_cast<const char*>(x) + row0 * rowbytes, valid_bytes, rowbytes, ldsrow, tile, lane);
        __syncthreads();
        if (active && i < n) out[i] = mixture_eval<T>(m, d, tile + lane * ldsrow);
        __syncthreads();
    }
}

// Flat form for rows of a power-of-two number (<= 64) of 16-byte pieces: one piece per thread, coalesced 16-byte loads with
// no LDS, the piece's coordinates' (mu, prec) of every component in registers for the whole grid-stride loop, quadratic forms
// completed by a butterfly over the row's lanes, log-sum-exp over the components by the row's first lane (same formula as
// mixture_eval; the quadratic form is summed in butterfly order instead of coordinate order: ~1e-16 relative).
template <typename T, int CMAX>
__global__ __launch_bounds__(ASMC_BLOCK) void k_mixture_flat(int64_t n, int d, int tpr_log2, const uint4* __restrict__ x, MixDev m,
                                                            double* __restrict__ out, const double* __restrict__ premap) {
    // premap != NULL (asmc_mixture_logpdf_premap): the density is evaluated at t_j = clip(a_j x_j + b_j, lo_j, hi_j) and
    // sum_j h_j t_j^2 is added; rows a, b, lo, hi, h of d doubles each
    constexpr int EPT = 16 / (int)sizeof(T);
    const int tpr = 1 << tpr_log2, C = m.C;
    const int64_t total = n << tpr_log2;
    const int64_t stride = (int64_t)gridDim.x * ASMC_BLOCK;  // a multiple of tpr: a thread keeps its coordinates
    const int c0 = (int)(((int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x) & (tpr - 1));
    double mu[CMAX][EPT], pr[CMAX][EPT];
#pragma unroll
    for (int c = 0; c < CMAX; c++)
#pragma unroll
        for (int k = 0; k < EPT; k++) {
            mu[c][k] = c < C ? m.mu[(size_t)c * d + c0 * EPT + k] : 0.0;
            pr[c][k] = c < C ? m.prec[(size_t)c * d + c0 * EPT + k] : 0.0;
        }
    double pa[EPT], pb[EPT], plo[EPT], phi[EPT], ph[EPT];
#pragma unroll
    for (int k = 0; k < EPT; k++) {
        const int j = c0 * EPT + k;
        pa[k] = premap ? premap[j] : 1.0;
        pb[k] = premap ? premap[d + j] : 0.0;
        plo[k] = premap ? premap[2 * d + j] : -INFINITY;
        phi[k] = premap ? premap[3 * d + j] : INFINITY;
        ph[k] = premap ? premap[4 * d + j] : 0.0;
    }
    for (int64_t e0 = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x; e0 - (threadIdx.x & 63) < total; e0 += stride) {
        const bool valid = e0 < total;
        double q[CMAX], extra = 0.0;
#pragma unroll
        for (int c = 0; c < CMAX; c++) q[c] = 0.0;
        if (valid) {
            const uint4 raw = x[e0];
            const T* vals = reinterpret_cast<const T*>(&raw);
            double xv[EPT];
#pragma unroll
            for (int k = 0; k < EPT; k++) {
                xv[k] = (double)vals[k];
                if (premap) {
                    xv[k] = clip(xv[k] * pa[k] + pb[k], plo[k], phi[k]);  // (NaN stays NaN: fmin / fmax would hand out a clamp end)
                    extra = fma(ph[k] * xv[k], xv[k], extra);
                }
            }
#pragma unroll
            for (int c = 0; c < CMAX; c++)
#pragma unroll
                for (int k = 0; k < EPT; k++) {
                    const double t = xv[k] - mu[c][k];
                    q[c] = fma(t * t, pr[c][k], q[c]);
                }
        }
#pragma unroll
        for (int c = 0; c < CMAX; c++)
            for (int o = tpr >> 1; o >= 1; o >>= 1) q[c] += __shfl_xor(q[c], o, 64);
        if (premap)
            for (int o = tpr >> 1; o >= 1; o >>= 1) extra += __shfl_xor(extra, o, 64);
        if (valid && c0 == 0) {
            double best = -INFINITY, terms[CMAX];
#pragma unroll
            for (int c = 0; c < CMAX; c++) {
                terms[c] = c < C ? m.logw[c] - 0.5 * q[c] : -INFINITY;
                best = fmax(best, terms[c]);
            }
            double r = terms[0];
            if (C > 1) {
                if (best == -INFINITY) {  // every term -inf or NaN: their sum (mixture_eval)
                    r = 0.0;
#pragma unroll
                    for (int c = 0; c < CMAX; c++)
                        if (c < C) r += terms[c];
                } else {
                    double ssum = 0.0;
#pragma unroll
                    for (int c = 0; c < CMAX; c++)
                        if (c < C) ssum += exp(terms[c] - best);
                    r = best + log(ssum);
                }
            }
            out[e0 >> tpr_log2] = r + extra;
        }
    }
}

extern "C" {

int asmc_gaussian_draw(asmc_ctx* ctx, int64_t n, int d, int x_dtype, const double* mu, const double* sigma,
                       uint64_t seed, uint64_t gid0, uint32_t draw_id, void* x_out, double* lq_out,
                       asmc_stream stream) {
    ASMC_REQUIRE(ctx && mu && sigma && x_out, "null pointer");
    ASMC_REQUIRE(n > 0 && d > 0 && d <= ASMC_MAX_DIMS, "bad sizes");
    ASMC_REQUIRE(x_dtype == ASMC_F64 || x_dtype == ASMC_F32, "bad x_dtype");
    hipStream_t st = as_stream(stream);
    const int grid = grid_for(n * ((d + 3) / 4), ASMC_BLOCK * 2, ASMC_MAX_BLOCKS * 2);
    const int grid2 = grid_for(n, ASMC_BLOCK, ASMC_MAX_BLOCKS * 2);
    if (x_dtype == ASMC_F64) {
        ASMC_LAUNCH(ctx, st, "k_gaussian_draw<double>", k_gaussian_draw<double>, dim3(grid), dim3(ASMC_BLOCK), 0, st, n, d, mu, sigma,
                           (unsigned long long)seed, (unsigned long long)gid0, draw_id, (double*)x_out, (const double*)ctx->d_bmtab);
        ASMC_LAUNCH_CHECK();
        if (lq_out) ASMC_LAUNCH(ctx, st, "k_gaussian_logq<double>", k_gaussian_logq<double>, dim3(grid2), dim3(ASMC_BLOCK), 0, st, n, d, mu, sigma, (const double*)x_out, lq_out);
    } else {
        ASMC_LAUNCH(ctx, st, "k_gaussian_draw<float>", k_gaussian_draw<float>, dim3(grid), dim3(ASMC_BLOCK), 0, st, n, d, mu, sigma,
                           (unsigned long long)seed, (unsigned long long)gid0, draw_id, (float*)x_out, (const double*)ctx->d_bmtab);
        ASMC_LAUNCH_CHECK();
        if (lq_out) ASMC_LAUNCH(ctx, st, "k_gaussian_logq<float>", k_gaussian_logq<float>, dim3(grid2), dim3(ASMC_BLOCK), 0, st, n, d, mu, sigma, (const float*)x_out, lq_out);
    }
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

static int mixture_logpdf_impl(asmc_ctx* ctx, int64_t n, int d, int x_dtype, const void* x, const asmc_mixture* density,
                               double* out, const double* premap, asmc_stream stream) {
    ASMC_REQUIRE(ctx && x && density && out, "null pointer");
    ASMC_REQUIRE(n > 0 && d > 0 && d <= ASMC_MAX_DIMS, "bad sizes");
    ASMC_REQUIRE(x_dtype == ASMC_F64 || x_dtype == ASMC_F32, "bad x_dtype");
    int rc = check_mixture(*density);
    if (rc) return rc;
    hipStream_t st = as_stream(stream);
    const int elem = x_dtype == ASMC_F64 ? 8 : 4;
    const int rowbytes = d * elem;
    size_t lds_bytes = 0;
    const int wpb = waves_for_lds((size_t)64 * lds_row_stride(rowbytes), &lds_bytes);
    const int64_t n_tiles = (n + 63) / 64;
    int cap = ctx->num_cu * 4;
    if (cap > ASMC_MAX_BLOCKS) cap = ASMC_MAX_BLOCKS;
    const int grid = grid_for(n_tiles, wpb, cap);
    const int vec = pick_vec(rowbytes, x, x);
    const MixDev m = to_dev(*density);
    {
        const int pieces = rowbytes / 16;
        if (rowbytes % 16 == 0 && ((uintptr_t)x % 16) == 0 && pieces >= 1 && pieces <= 64 && (pieces & (pieces - 1)) == 0 &&
            m.C <= 4 && !getenv("ASMC_MIXTURE_TILED")) {
            int lg = 0;
            while ((1 << lg) < pieces) lg++;
            const int g = grid_for(n * pieces, ASMC_BLOCK, ctx->num_cu * 32);
            if (x_dtype == ASMC_F64) {
                if (m.C == 1)
                    ASMC_LAUNCH(ctx, st, "k_mixture_logpdf", (k_mixture_flat<double, 1>), dim3(g), dim3(ASMC_BLOCK), 0, st, n, d, lg,
                                (const uint4*)x, m, out, premap);
                else
                    ASMC_LAUNCH(ctx, st, "k_mixture_logpdf", (k_mixture_flat<double, 4>), dim3(g), dim3(ASMC_BLOCK), 0, st, n, d, lg,
                                (const uint4*)x, m, out, premap);
            } else {
                if (m.C == 1)
                    ASMC_LAUNCH(ctx, st, "k_mixture_logpdf", (k_mixture_flat<float, 1>), dim3(g), dim3(ASMC_BLOCK), 0, st, n, d, lg,
                                (const uint4*)x, m, out, premap);
                else
                    ASMC_LAUNCH(ctx, st, "k_mixture_logpdf", (k_mixture_flat<float, 4>), dim3(g), dim3(ASMC_BLOCK), 0, st, n, d, lg,
                                (const uint4*)x, m, out, premap);
            }
            ASMC_LAUNCH_CHECK();
            return ASMC_OK;
        }
    }
    if (premap) {
        asmc_set_error("asmc_mixture_logpdf_premap: rows must be a power-of-two number (<= 64) of 16-byte pieces, <= 4 components");
        return ASMC_ERR_UNSUPPORTED;
    }
    auto launch = [&](auto kern, auto xp) {
        if (lds_bytes > 64 * 1024)
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        ASMC_LAUNCH(ctx, st, "k_mixture_logpdf", kern, dim3(grid), dim3(wpb * 64), lds_bytes, st, n, d, xp, m, out, wpb);
    };
    if (x_dtype == ASMC_F64) {
        const double* xp = (const double*)x;
        if (vec == 16) launch(k_mixture_logpdf<double, 16>, xp);
        else launch(k_mixture_logpdf<double, 8>, xp);
    } else {
        const float* xp = (const float*)x;
        if (vec == 16) launch(k_mixture_logpdf<float, 16>, xp);
        else if (vec == 8) launch(k_mixture_logpdf<float, 8>, xp);
        else launch(k_mixture_logpdf<float, 4>, xp);
    }
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int asmc_mixture_logpdf(asmc_ctx* ctx, int64_t n, int d, int x_dtype, const void* x, const asmc_mixture* density,
                        double* out, asmc_stream stream) {
    return mixture_logpdf_impl(ctx, n, d, x_dtype, x, density, out, nullptr, stream);
}

int asmc_mixture_logpdf_premap(asmc_ctx* ctx, int64_t n, int d, int x_dtype, const void* x, const double* premap_dev,
                               const asmc_mixture* density, double* out, asmc_stream stream) {
    ASMC_REQUIRE(premap_dev != nullptr, "null premap");
    return mixture_logpdf_impl(ctx, n, d, x_dtype, x, density, out, premap_dev, stream);
}

}  // extern "C"
