// asmc_weights_dev.h — the two device pieces the plain weight passes (asmc_weights.hip) share with the search files: the tempered
// log-weight and the body of the evidence-variance / second log-sum-exp pass.
#pragma once
#include "asmc_common.h"

__device__ __forceinline__ double lw_of(double ll, double lp, double lq, double c1, double c2) {
    // (self.beta - beta) * log_q + (beta - self.beta) * (log_likelihood + log_prior)
    double t1 = c1 * lq;
    double t2 = c2 * (ll + lp);
    return t1 + t2;
}

// ---- evidence variance + second log-sum-exp (k_weights_m2_lse, k_weights_m2_lse_shard) ------------------------------------------
// One grid-stride pass of blocks of ASMC_BLOCK: column 0: sum (exp(lw - m) - mean_u)^2 (samples.py:1230-1242); column 1:
// sum exp((lw + shift) - mp), the logsumexp of the SHIFTED log-weights (samples.py:1277 on samples.py:1244-1249); the block's two
// sums -> partials[2 blockIdx.x + {0, 1}].  `active` false: no particle is read, the sums are zero.
__device__ __forceinline__ void m2_lse_block(int64_t n, const double* __restrict__ ll, const double* __restrict__ lp,
                                             const double* __restrict__ lq, double c1, double c2, double m, double mean_u,
                                             double shift, double mp, bool active, double* __restrict__ partials) {
    double acc = 0.0, s1p = 0.0;
    const int64_t stride = (int64_t)gridDim.x * ASMC_BLOCK;
    if (active)
        for (int64_t i = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x; i < n; i += stride) {
            const double lw = lw_of(ll[i], lp[i], lq[i], c1, c2);
            const double dlt = exp(lw - m) - mean_u;
            acc += dlt * dlt;
            s1p += exp((lw + shift) - mp);
        }
    __shared__ double s_p[ASMC_BLOCK / 64][2];
    acc = wave_sum(acc);
    s1p = wave_sum(s1p);
    if ((threadIdx.x & 63) == 0) {
        s_p[threadIdx.x >> 6][0] = acc;
        s_p[threadIdx.x >> 6][1] = s1p;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        double v = s_p[0][threadIdx.x];
        for (int w = 1; w < ASMC_BLOCK / 64; w++) v += s_p[w][threadIdx.x];
        partials[(size_t)blockIdx.x * 2 + threadIdx.x] = v;
    }
}
