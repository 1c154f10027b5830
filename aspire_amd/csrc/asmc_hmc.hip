// asmc_hmc.hip — the mutations of the "blackjax_smc" sampler (reference src/aspire/samplers/smc/blackjax.py:145-349): random-walk
// Metropolis-Hastings and Hamiltonian Monte Carlo on the tempered log-target of smc/base.py:507-519, one independent chain per
// particle.  Specification and counter layout: include/asmc.h (asmc_rw_* / asmc_mh_* / asmc_hmc_*), DESIGN.md §3.13.
//
// Every particle gid = gid0 + i owns the pCN streams (asmc_pcn_dev.h): the normals of coordinates 4 q .. 4 q + 3 at transition t are
// normal_quad(seed, gid, t, q), the accept variate is accept_uniform(seed, gid, t).  The key (seed) differs per mutation.
//   k_hmc_mix        built-in densities (three diagonal Gaussian mixtures): whole HMC transitions, several per launch, out of
//                    registers - the particle is read once and written once per launch
//   k_rw_propose     y = x + sigma xi (scalar, diagonal or lower-triangular factor); also draws the momenta p = xi / sqrt(minv)
//   (caller)         densities at y, or gradients at z by torch.autograd between the leapfrog launches
//   k_mh_accept      symmetric Metropolis-Hastings accept, rows and carried densities in place
//   k_hmc_leap       p += kick g; z += drift minv p
//   k_hmc_accept     accept on dH = [log p_t(z') - K(p')] - [log p_t(z) - K(p)]
// The accepts of step index t go to the device-resident counter ctx->d_mh[t]; asmc_mh_counts reads a chunk of them back once.
#include "asmc_hmc_dev.h"

// (row layout, HmcMixArgs, hmc_row_sum / hmc_stage / hmc_mix_value_grad / hmc_target / hmc_kinetic: asmc_hmc_dev.h)
template <int LG, int NQ>
__global__ __launch_bounds__(ASMC_BLOCK, 2) void k_hmc_mix(double* __restrict__ x, double* __restrict__ ll, double* __restrict__ lp,
                                                        double* __restrict__ lq, const HmcMixArgs a, double* __restrict__ dH_out,
                                                        unsigned long long* __restrict__ counts) {
    constexpr int TPR = 1 << LG, NC = 4 * NQ, DPAD = NC * TPR, ROWS = ASMC_BLOCK >> LG;
    extern __shared__ __align__(16) double smem[];
    unsigned int* s_cnt = reinterpret_cast<unsigned int*>(smem);  // [n_steps] accepts of this block's rows per transition
    double* t_ll = smem + (a.n_steps + 1) / 2;
    double* t_lp = t_ll + ASMC_MAX_COMPONENTS + 2 * a.ll.C * DPAD;
    double* t_lq = t_lp + ASMC_MAX_COMPONENTS + 2 * a.lp.C * DPAD;
    bm_d2* bmt = bm_lds();
    bm_tab_stage<ASMC_BLOCK>(bmt, a.bmtab);
    hmc_stage<DPAD>(t_ll, a.ll, a.d);
    hmc_stage<DPAD>(t_lp, a.lp, a.d);
    hmc_stage<DPAD>(t_lq, a.lq, a.d);
    for (int s = threadIdx.x; s < a.n_steps; s += ASMC_BLOCK) s_cnt[s] = 0u;
    __syncthreads();

    const int lr = threadIdx.x & (TPR - 1), rib = threadIdx.x >> LG;
    double im[NC];  // diagonal of M^-1 (1 on the padding)
#pragma unroll
    for (int qi = 0; qi < NQ; qi++)
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int c = 4 * (lr + qi * TPR) + e;
            im[4 * qi + e] = (c < a.d && a.minv != nullptr) ? a.minv[c] : 1.0;
        }
    const int64_t n_tiles = (a.n + ROWS - 1) / ROWS;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row = tile * ROWS + rib;
        const bool valid = row < a.n;
        const unsigned long long gid = a.gid0 + (unsigned long long)row;
        double xc[NC], gc[NC];
#pragma unroll
        for (int qi = 0; qi < NQ; qi++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int c = 4 * (lr + qi * TPR) + e;
                xc[4 * qi + e] = (valid && c < a.d) ? x[row * a.d + c] : 0.0;
            }
        // the densities and the gradient at x are recomputed here, once per launch: the carried arrays are only written
        double vll, vlp, vlq;
        hmc_target<LG, NQ>(t_ll, t_lp, t_lq, a, lr, xc, vll, vlp, vlq, gc);
        bool moved = false;
        double dH = 0.0;
#pragma unroll 1
        for (int s = 0; s < a.n_steps; s++) {
            const uint32_t t = a.step0 + (uint32_t)s;
            double xn[NC], gn[NC], pn[NC];
#pragma unroll
            for (int qi = 0; qi < NQ; qi++) {
                double z0, z1, z2, z3;
                normal_quad(a.seed, gid, t, (uint32_t)(lr + qi * TPR), bmt, z0, z1, z2, z3);
                const double z[4] = {z0, z1, z2, z3};
#pragma unroll
                for (int e = 0; e < 4; e++)  // p ~ N(0, M); no momentum on the padding
                    pn[4 * qi + e] = 4 * (lr + qi * TPR) + e < a.d ? z[e] / sqrt(im[4 * qi + e]) : 0.0;
            }
            const double h0 = log_p_t(vll, vlp, vlq, a.beta) - hmc_kinetic<LG, NQ>(pn, im);
            const double half = 0.5 * a.eps;
#pragma unroll
            for (int j = 0; j < NC; j++) {
                pn[j] = pn[j] + half * gc[j];
                xn[j] = xc[j] + a.eps * (im[j] * pn[j]);
            }
            double nll, nlp, nlq;
#pragma unroll 1
            for (int i = 0; i < a.n_leap; i++) {
                hmc_target<LG, NQ>(t_ll, t_lp, t_lq, a, lr, xn, nll, nlp, nlq, gn);
                const bool last = i == a.n_leap - 1;
                const double kick = last ? half : a.eps, drift = last ? 0.0 : a.eps;
#pragma unroll
                for (int j = 0; j < NC; j++) {
                    pn[j] = pn[j] + kick * gn[j];
                    xn[j] = xn[j] + drift * (im[j] * pn[j]);
                }
            }
            const double h1 = log_p_t(nll, nlp, nlq, a.beta) - hmc_kinetic<LG, NQ>(pn, im);
            dH = h1 - h0;
            const bool acc = valid && log(accept_uniform(a.seed, gid, t)) < dH;  // NaN dH, NaN / +inf proposal target: rejected
            if (acc) {
#pragma unroll
                for (int j = 0; j < NC; j++) {
                    xc[j] = xn[j];
                    gc[j] = gn[j];
                }
                vll = nll;
                vlp = nlp;
                vlq = nlq;
                moved = true;
            }
            const unsigned long long b = __ballot(acc && lr == 0);
            if ((threadIdx.x & (ASMC_WAVE - 1)) == 0 && b != 0ull) atomicAdd(&s_cnt[s], (unsigned int)__popcll(b));
        }
        if (moved) {
#pragma unroll
            for (int qi = 0; qi < NQ; qi++)
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int c = 4 * (lr + qi * TPR) + e;
                    if (c < a.d) x[row * a.d + c] = xc[4 * qi + e];
                }
            if (lr == 0) {
                ll[row] = vll;
                lp[row] = vlp;
                lq[row] = vlq;
            }
        }
        if (dH_out != nullptr && valid && lr == 0) dH_out[row] = dH;
    }
    __syncthreads();
    for (int s = threadIdx.x; s < a.n_steps; s += ASMC_BLOCK)
        if (s_cnt[s] != 0u) atomicAdd(counts + s, (unsigned long long)s_cnt[s]);
}

// ---- split path ------------------------------------------------------------------------------------------------------------------
#define RW_SCALAR 0    // y = x + sigma xi
#define RW_DIAG 1      // y = x + sig[c] xi_c
#define RW_TRIL 2      // y = x + L xi, L = sig [d, d] row-major, lower triangle
#define RW_MOMENTUM 3  // y = xi_c / sqrt(sig[c]) (sig = diagonal of M^-1, nullptr: identity); x unused

struct RwArgs {
    int64_t n;
    int d, lg_tpr, mode;
    double sigma;
    const double* sig;
    unsigned long long seed, gid0;
    uint32_t step;
    const double* bmtab;
};

template <typename T>
__global__ __launch_bounds__(ASMC_BLOCK) void k_rw_propose(const T* __restrict__ x, T* __restrict__ y, const RwArgs a,
                                                           unsigned long long* __restrict__ count) {
    extern __shared__ __align__(16) double s_xi[];  // RW_TRIL: [rows of the block][4 ceil(d / 4)] normals
    bm_d2* bmt = bm_lds();
    bm_tab_stage<ASMC_BLOCK>(bmt, a.bmtab);
    if (count != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *count = 0;  // the step's first launch opens its counter
    __syncthreads();
    const int tpr = 1 << a.lg_tpr, lr = threadIdx.x & (tpr - 1), rib = threadIdx.x >> a.lg_tpr;
    const int64_t row = (int64_t)blockIdx.x * (ASMC_BLOCK >> a.lg_tpr) + rib;
    const bool valid = row < a.n;
    const int nq = (a.d + 3) / 4, dq = 4 * nq;
    if (valid) {
        for (int q = lr; q < nq; q += tpr) {
            double z[4];
            normal_quad(a.seed, a.gid0 + (unsigned long long)row, a.step, (uint32_t)q, bmt, z[0], z[1], z[2], z[3]);
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int c = 4 * q + e;
                if (a.mode == RW_TRIL) {
                    s_xi[rib * dq + c] = z[e];
                } else if (c < a.d) {
                    const int64_t o = row * a.d + c;
                    if (a.mode == RW_MOMENTUM) {
                        y[o] = (T)(a.sig != nullptr ? z[e] / sqrt(a.sig[c]) : z[e]);
                    } else {
                        const double s = a.mode == RW_SCALAR ? a.sigma : a.sig[c];
                        y[o] = (T)((double)x[o] + s * z[e]);
                    }
                }
            }
        }
    }
    if (a.mode == RW_TRIL) {
        __syncthreads();
        if (valid) {
            const double* __restrict__ xi = s_xi + rib * dq;
            for (int c = lr; c < a.d; c += tpr) {
                const double* __restrict__ Lc = a.sig + (size_t)c * a.d;
                double acc = 0.0;
                for (int j = 0; j <= c; j++) acc = fma(Lc[j], xi[j], acc);
                y[row * a.d + c] = (T)((double)x[row * a.d + c] + acc);
            }
        }
    }
}

// rows of y (TY) into the accepted rows of x (TX): s_acc[r] of the block's rows, 2^lg_tpr lanes per row
template <typename TX, typename TY>
__device__ __forceinline__ void mh_copy_rows(TX* __restrict__ x, const TY* __restrict__ y, const unsigned char* s_acc, int64_t i0,
                                             int64_t n, int d, int lg_tpr) {
    const int64_t rows = n - i0 < ASMC_BLOCK ? n - i0 : ASMC_BLOCK;
    const int tpr = 1 << lg_tpr;
    for (int64_t r = threadIdx.x >> lg_tpr; r < rows; r += ASMC_BLOCK >> lg_tpr) {
        if (!s_acc[r]) continue;
        const TY* __restrict__ yr = y + (i0 + r) * d;
        TX* __restrict__ xr = x + (i0 + r) * d;
        for (int c = threadIdx.x & (tpr - 1); c < d; c += tpr) xr[c] = (TX)yr[c];
    }
}

template <typename T>
__global__ __launch_bounds__(ASMC_BLOCK) void k_mh_accept(T* __restrict__ x, const T* __restrict__ y, int64_t n, int d, int lg_tpr,
                                                          double beta, double* __restrict__ ll, double* __restrict__ lp,
                                                          double* __restrict__ lq, double* __restrict__ lj,
                                                          const double* __restrict__ ll_new, const double* __restrict__ lp_new,
                                                          const double* __restrict__ lq_new, const double* __restrict__ lj_new,
                                                          unsigned long long seed, unsigned long long gid0, uint32_t step,
                                                          unsigned long long* __restrict__ count) {
    __shared__ unsigned char s_acc[ASMC_BLOCK];
    const int64_t i0 = (int64_t)blockIdx.x * ASMC_BLOCK;
    const int64_t i = i0 + threadIdx.x;
    bool acc = false;
    if (i < n) {
        double nlp = log_p_t(ll_new[i], lp_new[i], lq_new[i], beta);
        double olp = log_p_t(ll[i], lp[i], lq[i], beta);
        if (lj != nullptr) {  // a chain in a preconditioned space: log|det dT^-1/dz| joins the log-target, NaN / +inf -> -inf again
            nlp = log_p_t_guard(nlp + lj_new[i]);
            olp = log_p_t_guard(olp + lj[i]);
        }
        acc = nlp - olp > log(accept_uniform(seed, gid0 + (unsigned long long)i, step));
        if (acc) {
            ll[i] = ll_new[i];
            lp[i] = lp_new[i];
            lq[i] = lq_new[i];
            if (lj != nullptr) lj[i] = lj_new[i];
        }
    }
    s_acc[threadIdx.x] = acc;
    const unsigned long long ballot = __ballot(acc);
    if ((threadIdx.x & (ASMC_WAVE - 1)) == 0 && ballot != 0ull) atomicAdd(count, (unsigned long long)__popcll(ballot));
    __syncthreads();
    mh_copy_rows(x, y, s_acc, i0, n, d, lg_tpr);
}

__global__ __launch_bounds__(ASMC_BLOCK) void k_hmc_leap(double* __restrict__ z, double* __restrict__ p, const double* __restrict__ g,
                                                         const double* __restrict__ minv, int64_t total, int d, double kick, double drift) {
    for (int64_t e = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * ASMC_BLOCK) {
        const double pe = p[e] + kick * g[e];
        p[e] = pe;
        const double im = minv != nullptr ? minv[e % d] : 1.0;
        z[e] = z[e] + drift * (im * pe);
    }
}

template <typename T>
__global__ __launch_bounds__(ASMC_BLOCK) void k_hmc_accept(T* __restrict__ x, const double* __restrict__ z_new, const double* __restrict__ p0,
                                                           const double* __restrict__ p1, const double* __restrict__ minv,
                                                           const double* __restrict__ ke0, const double* __restrict__ ke1, int64_t n, int d,
                                                           int lg_tpr, double beta, double* __restrict__ ll, double* __restrict__ lp,
                                                           double* __restrict__ lq, const double* __restrict__ ll_new,
                                                           const double* __restrict__ lp_new, const double* __restrict__ lq_new,
                                                           unsigned long long seed, unsigned long long gid0, uint32_t step,
                                                           unsigned char* __restrict__ flags, double* __restrict__ dH_out,
                                                           unsigned long long* __restrict__ count) {
    __shared__ unsigned char s_acc[ASMC_BLOCK];
    const int64_t i0 = (int64_t)blockIdx.x * ASMC_BLOCK;
    const int64_t i = i0 + threadIdx.x;
    bool acc = false;
    if (i < n) {
        double k0, k1;
        if (ke0 != nullptr) {
            k0 = ke0[i];
            k1 = ke1[i];
        } else {  // K = 1/2 p^T M^-1 p
            k0 = 0.0;
            k1 = 0.0;
            for (int j = 0; j < d; j++) {
                const double im = minv != nullptr ? minv[j] : 1.0;
                const double a = p0[i * d + j], b = p1[i * d + j];
                k0 = fma(im * a, a, k0);
                k1 = fma(im * b, b, k1);
            }
            k0 *= 0.5;
            k1 *= 0.5;
        }
        const double h0 = log_p_t(ll[i], lp[i], lq[i], beta) - k0;
        const double h1 = log_p_t(ll_new[i], lp_new[i], lq_new[i], beta) - k1;
        const double dH = h1 - h0;
        acc = log(accept_uniform(seed, gid0 + (unsigned long long)i, step)) < dH;  // NaN dH, NaN / +inf proposal target: rejected
        if (acc) {
            ll[i] = ll_new[i];
            lp[i] = lp_new[i];
            lq[i] = lq_new[i];
        }
        if (flags != nullptr) flags[i] = acc;
        if (dH_out != nullptr) dH_out[i] = dH;
    }
    s_acc[threadIdx.x] = acc;
    const unsigned long long ballot = __ballot(acc);
    if ((threadIdx.x & (ASMC_WAVE - 1)) == 0 && ballot != 0ull) atomicAdd(count, (unsigned long long)__popcll(ballot));
    __syncthreads();
    mh_copy_rows(x, z_new, s_acc, i0, n, d, lg_tpr);
}

static int mh_common(asmc_ctx* ctx, int64_t n, int d, int t, const char* who) {
    if (ctx == nullptr || !(n >= 1 && n < (1LL << 31) && d > 0 && d <= ASMC_MAX_DIMS) || !(t >= 0 && t < ASMC_MAX_PCN_STEPS)) {
        asmc_set_error("%s: bad arguments (ctx, 1 <= n < 2^31, 0 < d <= ASMC_MAX_DIMS, 0 <= t < ASMC_MAX_PCN_STEPS)", who);
        return ASMC_ERR_ARG;
    }
    return ASMC_OK;
}

static int lg_lanes(int items) {  // log2 of the lanes that share a row: the smallest power of two >= items, at most a wave
    int lg = 0;
    while ((1 << lg) < items && lg < 6) lg++;
    return lg;
}

static int rw_launch(asmc_ctx* ctx, int64_t n, int d, int x_dtype, const void* x, int mode, double sigma, const double* sig,
                     uint64_t seed, uint64_t gid0, uint32_t step, int t, void* y, hipStream_t st) {
    RwArgs a;
    memset(&a, 0, sizeof(a));
    a.n = n;
    a.d = d;
    a.lg_tpr = lg_lanes((d + 3) / 4);
    a.mode = mode;
    a.sigma = sigma;
    a.sig = sig;
    a.seed = seed;
    a.gid0 = gid0;
    a.step = step;
    a.bmtab = ctx->d_bmtab;
    const int rows = ASMC_BLOCK >> a.lg_tpr;
    const int grid = (int)((n + rows - 1) / rows);
    const size_t lds = mode == RW_TRIL ? sizeof(double) * rows * 4 * ((d + 3) / 4) : 0;
    if (x_dtype == ASMC_F64)
        ASMC_LAUNCH(ctx, st, "k_rw_propose", k_rw_propose<double>, dim3(grid), dim3(ASMC_BLOCK), lds, st, (const double*)x, (double*)y, a,
                    ctx->d_mh + t);
    else
        ASMC_LAUNCH(ctx, st, "k_rw_propose", k_rw_propose<float>, dim3(grid), dim3(ASMC_BLOCK), lds, st, (const float*)x, (float*)y, a,
                    ctx->d_mh + t);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

template <int LG, int NQ>
static int hmc_mix_launch(asmc_ctx* ctx, double* x, double* ll, double* lp, double* lq, const HmcMixArgs& a, double* dH_out,
                          unsigned long long* counts, hipStream_t st) {
    constexpr int DPAD = 4 * NQ * (1 << LG), ROWS = ASMC_BLOCK >> LG;
    const size_t lds = sizeof(double) * ((a.n_steps + 1) / 2 + 3 * ASMC_MAX_COMPONENTS + 2 * DPAD * (a.ll.C + a.lp.C + a.lq.C));
    const int64_t tiles = (a.n + ROWS - 1) / ROWS;
    const int64_t cap = (int64_t)ctx->num_cu * 8;
    const int grid = (int)(tiles < cap ? tiles : cap);
    ASMC_LAUNCH(ctx, st, "k_hmc_mix", (k_hmc_mix<LG, NQ>), dim3(grid), dim3(ASMC_BLOCK), lds, st, x, ll, lp, lq, a, dH_out, counts);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

extern "C" {

int asmc_rw_propose(asmc_ctx* ctx, int64_t n, int d, int x_dtype, const void* x, int sigma_mode, double sigma, const double* sig,
                    uint64_t seed, uint64_t gid0, uint32_t step, int t, void* y, asmc_stream stream) {
    const int rc = mh_common(ctx, n, d, t, __func__);
    if (rc) return rc;
    ASMC_REQUIRE(x_dtype == ASMC_F64 || x_dtype == ASMC_F32, "bad x_dtype");
    ASMC_REQUIRE(x && y, "null pointer");
    ASMC_REQUIRE(sigma_mode == RW_SCALAR || ((sigma_mode == RW_DIAG || sigma_mode == RW_TRIL) && sig != nullptr),
                 "sigma_mode must be 0 (scalar), 1 (diagonal) or 2 (lower-triangular factor), the last two with sig_dev");
    return rw_launch(ctx, n, d, x_dtype, x, sigma_mode, sigma, sig, seed, gid0, step, t, y, as_stream(stream));
}

int asmc_hmc_momentum(asmc_ctx* ctx, int64_t n, int d, const double* minv, uint64_t seed, uint64_t gid0, uint32_t step, int t,
                      double* p, asmc_stream stream) {
    const int rc = mh_common(ctx, n, d, t, __func__);
    if (rc) return rc;
    ASMC_REQUIRE(p, "null pointer");
    return rw_launch(ctx, n, d, ASMC_F64, nullptr, RW_MOMENTUM, 0.0, minv, seed, gid0, step, t, p, as_stream(stream));
}

int asmc_mh_accept(asmc_ctx* ctx, int64_t n, int d, int x_dtype, void* x, const void* y, double beta, double* ll, double* lp,
                   double* lq, double* lj, const double* ll_new, const double* lp_new, const double* lq_new, const double* lj_new,
                   uint64_t seed, uint64_t gid0, uint32_t step, int t, asmc_stream stream) {
    const int rc = mh_common(ctx, n, d, t, __func__);
    if (rc) return rc;
    ASMC_REQUIRE(x_dtype == ASMC_F64 || x_dtype == ASMC_F32, "bad x_dtype");
    ASMC_REQUIRE(x && y && ll && lp && lq && ll_new && lp_new && lq_new, "null pointer");
    ASMC_REQUIRE((lj == nullptr) == (lj_new == nullptr), "log-Jacobian arrays: both or neither");
    hipStream_t st = as_stream(stream);
    const int grid = (int)((n + ASMC_BLOCK - 1) / ASMC_BLOCK);
    const int lg = lg_lanes(d);
    if (x_dtype == ASMC_F64)
        ASMC_LAUNCH(ctx, st, "k_mh_accept", k_mh_accept<double>, dim3(grid), dim3(ASMC_BLOCK), 0, st, (double*)x, (const double*)y, n, d,
                    lg, beta, ll, lp, lq, lj, ll_new, lp_new, lq_new, lj_new, seed, gid0, step, ctx->d_mh + t);
    else
        ASMC_LAUNCH(ctx, st, "k_mh_accept", k_mh_accept<float>, dim3(grid), dim3(ASMC_BLOCK), 0, st, (float*)x, (const float*)y, n, d, lg,
                    beta, ll, lp, lq, lj, ll_new, lp_new, lq_new, lj_new, seed, gid0, step, ctx->d_mh + t);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int asmc_hmc_leap(asmc_ctx* ctx, int64_t n, int d, double* z, double* p, const double* g, const double* minv, double kick,
                  double drift, asmc_stream stream) {
    const int rc = mh_common(ctx, n, d, 0, __func__);
    if (rc) return rc;
    ASMC_REQUIRE(z && p && g, "null pointer");
    hipStream_t st = as_stream(stream);
    const int64_t total = n * d;
    ASMC_LAUNCH(ctx, st, "k_hmc_leap", k_hmc_leap, dim3(grid_for(total, ASMC_BLOCK, ctx->num_cu * 32)), dim3(ASMC_BLOCK), 0, st, z, p, g,
                minv, total, d, kick, drift);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int asmc_hmc_accept(asmc_ctx* ctx, int64_t n, int d, int x_dtype, void* x, const double* z_new, const double* p0, const double* p1,
                    const double* minv, const double* ke0, const double* ke1, double beta, double* ll, double* lp, double* lq,
                    const double* ll_new, const double* lp_new, const double* lq_new, uint64_t seed, uint64_t gid0, uint32_t step,
                    int t, unsigned char* flags, double* dH_out, asmc_stream stream) {
    const int rc = mh_common(ctx, n, d, t, __func__);
    if (rc) return rc;
    ASMC_REQUIRE(x_dtype == ASMC_F64 || x_dtype == ASMC_F32, "bad x_dtype");
    ASMC_REQUIRE(x && z_new && ll && lp && lq && ll_new && lp_new && lq_new, "null pointer");
    ASMC_REQUIRE((ke0 == nullptr) == (ke1 == nullptr), "kinetic energies: both or neither");
    ASMC_REQUIRE(ke0 != nullptr || (p0 != nullptr && p1 != nullptr), "either the kinetic energies or both momenta");
    hipStream_t st = as_stream(stream);
    const int grid = (int)((n + ASMC_BLOCK - 1) / ASMC_BLOCK);
    const int lg = lg_lanes(d);
    if (x_dtype == ASMC_F64)
        ASMC_LAUNCH(ctx, st, "k_hmc_accept", k_hmc_accept<double>, dim3(grid), dim3(ASMC_BLOCK), 0, st, (double*)x, z_new, p0, p1, minv,
                    ke0, ke1, n, d, lg, beta, ll, lp, lq, ll_new, lp_new, lq_new, seed, gid0, step, flags, dH_out, ctx->d_mh + t);
    else
        ASMC_LAUNCH(ctx, st, "k_hmc_accept", k_hmc_accept<float>, dim3(grid), dim3(ASMC_BLOCK), 0, st, (float*)x, z_new, p0, p1, minv, ke0,
                    ke1, n, d, lg, beta, ll, lp, lq, ll_new, lp_new, lq_new, seed, gid0, step, flags, dH_out, ctx->d_mh + t);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int asmc_hmc_mix(asmc_ctx* ctx, int64_t n, int d, void* x, double* ll, double* lp, double* lq, double beta,
                 const asmc_mixture* log_likelihood, const asmc_mixture* log_prior, const asmc_mixture* log_q, const double* minv,
                 double step_size, int n_leap, uint64_t seed, uint64_t gid0, uint32_t step0, int n_steps, int t0, double* dH_out,
                 asmc_stream stream) {
    const int rc = mh_common(ctx, n, d, t0, __func__);
    if (rc) return rc;
    ASMC_REQUIRE(d <= HMC_FUSED_MAX_D, "the fused kernel covers d <= 128");
    ASMC_REQUIRE(x && ll && lp && lq && log_likelihood && log_prior && log_q, "null pointer");
    ASMC_REQUIRE(n_steps >= 1 && t0 + n_steps <= ASMC_MAX_PCN_STEPS, "step indices out of range");
    ASMC_REQUIRE(n_leap >= 1, "num_integration_steps must be >= 1");
    HmcMixArgs a;
    memset(&a, 0, sizeof(a));
    a.ll = to_dev(*log_likelihood);
    a.lp = to_dev(*log_prior);
    a.lq = to_dev(*log_q);
    for (const MixDev* m : {&a.ll, &a.lp, &a.lq})
        ASMC_REQUIRE(m->C >= 1 && m->C <= ASMC_MAX_COMPONENTS && m->logw && m->mu && m->prec, "bad mixture");
    a.n = n;
    a.d = d;
    a.n_steps = n_steps;
    a.n_leap = n_leap;
    a.step0 = step0;
    a.eps = step_size;
    a.beta = beta;
    a.seed = seed;
    a.gid0 = gid0;
    a.minv = minv;
    a.bmtab = ctx->d_bmtab;
    hipStream_t st = as_stream(stream);
    unsigned long long* counts = ctx->d_mh + t0;
    ASMC_HIP(hipMemsetAsync(counts, 0, sizeof(unsigned long long) * n_steps, st));
    double* xd = (double*)x;
    if (d <= 4) return hmc_mix_launch<0, 1>(ctx, xd, ll, lp, lq, a, dH_out, counts, st);
    if (d <= 8) return hmc_mix_launch<1, 1>(ctx, xd, ll, lp, lq, a, dH_out, counts, st);
    if (d <= 16) return hmc_mix_launch<2, 1>(ctx, xd, ll, lp, lq, a, dH_out, counts, st);
    if (d <= 32) return hmc_mix_launch<3, 1>(ctx, xd, ll, lp, lq, a, dH_out, counts, st);
    if (d <= 64) return hmc_mix_launch<3, 2>(ctx, xd, ll, lp, lq, a, dH_out, counts, st);
    return hmc_mix_launch<4, 2>(ctx, xd, ll, lp, lq, a, dH_out, counts, st);
}

int asmc_mh_counts(asmc_ctx* ctx, int n_steps, int64_t* counts_host, asmc_stream stream) {
    ASMC_REQUIRE(ctx && counts_host, "null pointer");
    ASMC_REQUIRE(n_steps >= 1 && n_steps <= ASMC_MAX_PCN_STEPS, "n_steps out of range");
    hipStream_t st = as_stream(stream);
    unsigned long long* h = reinterpret_cast<unsigned long long*>(ctx->h_pinned);
    ASMC_HIP(hipStreamSynchronize(st));  // pinned staging may still be in flight
    ASMC_HIP(hipMemcpyAsync(h, ctx->d_mh, sizeof(unsigned long long) * n_steps, hipMemcpyDeviceToHost, st));
    ASMC_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < n_steps; i++) counts_host[i] = (int64_t)h[i];
    return ASMC_OK;
}

}  // extern "C"
