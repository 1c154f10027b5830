// asmc_hmc_dev.h — device helpers shared by the fused HMC kernel (asmc_hmc.hip k_hmc_mix) and the fused NUTS kernel (asmc_nuts.hip
// k_nuts_mix): the quad row layout, the staged mixture tables, value and gradient of the tempered log-target, the kinetic energy.
#pragma once
#include "asmc_pcn_dev.h"

#define HMC_FUSED_MAX_D 128

// ---- fused HMC on three diagonal Gaussian mixtures ----------------------------------------------------------------------------
// Row layout: 2^LG lanes share a row, lane lr of them holds NQ quads of coordinates: quad q = lr + qi 2^LG, coordinates 4 q .. 4 q + 3
// (the unit is the quad of one Philox block, so every lane draws exactly the blocks it consumes and reads 32 contiguous bytes).
// Coordinates >= d are padding: x = p = 0 there and the staged tables hold mu = prec = 0, so no loop tests for them.
struct HmcMixArgs {
    int64_t n;
    int d, n_steps, n_leap;
    uint32_t step0;
    double eps, beta;
    unsigned long long seed, gid0;
    MixDev ll, lp, lq;
    const double* minv;   // [d] diagonal of the inverse mass matrix, nullptr: identity
    const double* bmtab;  // the Box-Muller tables in HBM
};

template <int LG>
__device__ __forceinline__ double hmc_row_sum(double v) {
#pragma unroll
    for (int o = (1 << LG) >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);  // a butterfly: every lane of the row ends with the same bits
    return v;
}

// LDS image of one mixture: logw[8] | mu[C][DPAD] | prec[C][DPAD]
template <int DPAD>
__device__ __forceinline__ void hmc_stage(double* __restrict__ t, const MixDev& m, int d) {
    for (int e = threadIdx.x; e < ASMC_MAX_COMPONENTS; e += ASMC_BLOCK) t[e] = e < m.C ? m.logw[e] : -INFINITY;
    const int tot = m.C * DPAD;
    for (int e = threadIdx.x; e < tot; e += ASMC_BLOCK) {
        const int c = e / DPAD, j = e - c * DPAD;
        t[ASMC_MAX_COMPONENTS + e] = j < d ? m.mu[(size_t)c * d + j] : 0.0;
        t[ASMC_MAX_COMPONENTS + tot + e] = j < d ? m.prec[(size_t)c * d + j] : 0.0;
    }
}

// log f(x) of one mixture; g += coef * grad log f(x).  t_c = logw_c - 1/2 sum_j prec_cj (x_j - mu_cj)^2, log f = logsumexp_c t_c,
// grad log f = -sum_c softmax(t)_c prec_c (x - mu_c): value and gradient in the same pass over the table.
template <int LG, int NQ>
__device__ __forceinline__ double hmc_mix_value_grad(const double* __restrict__ tab, int C, int lr, const double (&x)[4 * NQ], double coef,
                                                     double (&g)[4 * NQ]) {
    constexpr int TPR = 1 << LG, DPAD = 4 * NQ * TPR;
    const double* __restrict__ mu = tab + ASMC_MAX_COMPONENTS + 4 * lr;
    const double* __restrict__ pr = mu + C * DPAD;
    if (C == 1) {
        double q = 0.0;
#pragma unroll
        for (int qi = 0; qi < NQ; qi++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int j = 4 * qi + e, o = 4 * qi * TPR + e;
                const double t = x[j] - mu[o];
                const double tp = pr[o] * t;
                q = fma(t, tp, q);
                g[j] = fma(-coef, tp, g[j]);
            }
        return tab[0] - 0.5 * hmc_row_sum<LG>(q);
    }
    // running maximum m, s = sum_c exp(t_c - m) and ga = sum_c exp(t_c - m) prec_c (x - mu_c), rescaled when m grows: one pass over
    // the table, nothing per component kept
    double m = -INFINITY, s = 0.0;
    double ga[4 * NQ];
#pragma unroll
    for (int j = 0; j < 4 * NQ; j++) ga[j] = 0.0;
#pragma unroll 1
    for (int c = 0; c < C; c++) {
        double tp[4 * NQ];
        double q = 0.0;
#pragma unroll
        for (int qi = 0; qi < NQ; qi++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int j = 4 * qi + e, o = c * DPAD + 4 * qi * TPR + e;
                const double t = x[j] - mu[o];
                tp[j] = pr[o] * t;
                q = fma(t, tp[j], q);
            }
        const double tc = tab[c] - 0.5 * hmc_row_sum<LG>(q);
        const double mn = fmax(m, tc);
        const double scale = exp(m - mn), w = exp(tc - mn);
        s = fma(s, scale, w);
#pragma unroll
        for (int j = 0; j < 4 * NQ; j++) ga[j] = fma(ga[j], scale, w * tp[j]);
        m = mn;
    }
    const double inv = coef / s;
#pragma unroll
    for (int j = 0; j < 4 * NQ; j++) g[j] = fma(-inv, ga[j], g[j]);
    return m + log(s);
}

// the three densities at x and the gradient of (1 - beta) log q + beta (ll + lp)
template <int LG, int NQ>
__device__ __forceinline__ void hmc_target(const double* __restrict__ t_ll, const double* __restrict__ t_lp, const double* __restrict__ t_lq,
                                           const HmcMixArgs& a, int lr, const double (&x)[4 * NQ], double& vll, double& vlp, double& vlq,
                                           double (&g)[4 * NQ]) {
#pragma unroll
    for (int j = 0; j < 4 * NQ; j++) g[j] = 0.0;
    vll = hmc_mix_value_grad<LG, NQ>(t_ll, a.ll.C, lr, x, a.beta, g);
    vlp = hmc_mix_value_grad<LG, NQ>(t_lp, a.lp.C, lr, x, a.beta, g);
    vlq = hmc_mix_value_grad<LG, NQ>(t_lq, a.lq.C, lr, x, 1.0 - a.beta, g);
}

template <int LG, int NQ>
__device__ __forceinline__ double hmc_kinetic(const double (&p)[4 * NQ], const double (&im)[4 * NQ]) {
    double k = 0.0;
#pragma unroll
    for (int j = 0; j < 4 * NQ; j++) k = fma(im[j] * p[j], p[j], k);
    return 0.5 * hmc_row_sum<LG>(k);
}
