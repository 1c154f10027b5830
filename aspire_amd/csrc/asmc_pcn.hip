// asmc_pcn.hip — pCN mutation: the step kernels, their launchers (the templates, and in front of them the non-template launch
// functions that the drivers of asmc_pcn_drive.hip call: asmc_pcn_shared.h), the mutation read-back, the zero-padding scheme.
// (The proposal draw and the built-in densities live in asmc_density.hip, the population moments and the reference fit in
// asmc_moments.hip; asmc_pcn_shared.h holds what they share with this file.)
//
// Replaces (reference mj-will/aspire):
//   src/aspire/samplers/smc/minipcn.py:69-135  MiniPCNSMC.mutate  (wraps third-party minipcn —
//       absent from the reference tree; the kernel below implements THIS repository's pCN
//       specification; parity with minipcn is unpinned)
//   src/aspire/samplers/smc/base.py:507-519 + src/aspire/samples.py:1217-1219  tempered target
//       log p_t = (1-beta) log_q + beta (log_likelihood + log_prior) [+ log|J|], NaN -> -inf
//
// Data movement: particle rows (d*s bytes, particle-major) are fetched with fully coalesced
// 16-B-per-lane loads into a padded LDS tile (64 rows per wave, row stride = rowbytes + 16 so that
// per-lane row reads are bank-conflict free), processed one particle per lane, and written back
// coalesced from the same tile.  Noise is generated in-kernel (Philox4x32-10 + Box-Muller), so one
// pCN step moves 2*d*s + 48 bytes per particle and nothing else.
#include <stdlib.h>

#include <chrono>

#include "asmc_pcn_shared.h"
#include "asmc_pcn_reg.h"  // the register-resident step body (row_to_regs .. pcn_reg_body) and pcn_pack_block
#include "asmc_transform_dev.h"

// =============================================================================================
// fused pCN step, generic in d: per-lane work vector v[k] lives in LDS (SoA: v[k*64 + lane])
// =============================================================================================

// PHASE 0: fused (propose + built-in targets + accept, in place)
// PHASE 1: propose only (writes x_prop tile, qform_old, qform_new)
template <typename T, int VEC, int PHASE>
__global__ __launch_bounds__(ASMC_BLOCK) void k_pcn_step(
    int64_t n, T* __restrict__ x, double* __restrict__ ll, double* __restrict__ lp, double* __restrict__ lq,
    PcnDev p, const double* __restrict__ rho_ptr, uint32_t step, long long* __restrict__ block_counts,
    T* __restrict__ x_prop, double* __restrict__ qf_old, double* __restrict__ qf_new, int waves_per_block) {
    extern __shared__ __align__(16) char smem[];
    const int d = p.d;
    const int rowbytes = d * (int)sizeof(T);
    const int ldsrow = lds_row_stride(rowbytes);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wave_bytes = 64 * ldsrow + 64 * 8 * d;
    char* tile = smem + (size_t)wave * wave_bytes;
    double* v = reinterpret_cast<double*>(tile + 64 * ldsrow) + lane;  // v[k*64]
    char* myrow = tile + lane * ldsrow;
    const double rho = *rho_ptr;
    const double a = sqrt(1.0 - rho * rho);
    long long n_acc = 0;
    const int64_t n_tiles = (n + 63) / 64;
    bm_d2* bmt = bm_lds();  // the Box-Muller tables (the first tile's __syncthreads publishes them)
    bm_tab_stage_rt(bmt, p.bmtab);
    for (int64_t tile0 = (int64_t)blockIdx.x * waves_per_block; tile0 < n_tiles;
         tile0 += (int64_t)gridDim.x * waves_per_block) {
        const int64_t t = tile0 + wave;
        const bool active = t < n_tiles;
        const int64_t i = t * 64 + lane;
        const bool valid = active && i < n;
        const int64_t row0 = t * 64;
        const int64_t valid_bytes = active ? (((n - row0) < 64 ? (n - row0) : 64) * (int64_t)rowbytes) : 0;
        if (active) tile_load<VEC>(reinterpret_cast<const char*>(x) + row0 * rowbytes, valid_bytes, rowbytes, ldsrow, tile, lane);
        __syncthreads();
        bool acc = false;
        if (valid) {
            const unsigned long long gid = p.gid0 + (unsigned long long)i;
            // dx -> v
            for (int j = 0; j < d; j++) v[j * 64] = row_get<T>(myrow, j) - p.mu[j];
            // y = Linv dx (in place, descending rows), q0 = |y|^2
            double q0 = 0.0;
            for (int j = d - 1; j >= 0; j--) {
                const double* Lr = p.Linv + (size_t)j * d;
                double s = 0.0;
                for (int k = 0; k <= j; k++) s = fma(Lr[k], v[k * 64], s);
                v[j * 64] = s;
                q0 = fma(s, s, q0);
            }
            // y' = a y + rho sqrt(s) xi (s = 1 for the Gaussian reference), q1 = |y'|^2
            double q1 = 0.0;
            const double rs = tpcn_scale(rho, p.nu, q0, p.gam, i);
            const bool fast_noise = p.noise == ASMC_NOISE_F32;  // wave-uniform: the same stream as the register-resident kernels
            for (int qd = 0; 4 * qd < d; qd++) {
                double z[4];
                if (fast_noise)
                    normal_quad_f32(p.seed, gid, step, (uint32_t)qd, z[0], z[1], z[2], z[3]);
                else
                    normal_quad(p.seed, gid, step, (uint32_t)qd, bmt, z[0], z[1], z[2], z[3]);
                for (int e = 0; e < 4 && 4 * qd + e < d; e++) {
                    const double ye = fma(rs, z[e], a * v[(4 * qd + e) * 64]);
                    v[(4 * qd + e) * 64] = ye;
                    q1 = fma(ye, ye, q1);
                }
            }
            // x' = mu + L y' (in place, descending rows); rounded to the storage type
            for (int j = d - 1; j >= 0; j--) {
                const double* Lr = p.L + (size_t)j * d;
                double s = 0.0;
                for (int k = 0; k <= j; k++) s = fma(Lr[k], v[k * 64], s);
                v[j * 64] = (double)(T)(p.mu[j] + s);
            }
            if (PHASE == 1) {
                // the accept kernel adds half of these to the tempered log-targets: twice the reference's correction
                qf_old[i] = 2.0 * ref_corr(q0, p.nu, d);
                qf_new[i] = 2.0 * ref_corr(q1, p.nu, d);
                for (int j = 0; j < d; j++) row_set<T>(myrow, j, v[j * 64]);
            } else {
                // the old row is still in `myrow`; stage x' into it only on acceptance, so evaluate
                // the targets from a scratch copy: write x' to the row AFTER saving nothing — the old
                // row is not needed again (old ll/lp/lq come from HBM), so overwrite and restore on reject
                const double oll = ll[i], olp = lp[i], olq = lq[i];
                // evaluate the built-in targets at x' directly from the work vector via a temp row view
                double nll, nlp, nlq;
                {
                    // temporarily keep the old row in registers-free form: swap through LDS element-wise
                    // (row <- x', v <- old x) so mixture_eval can read a contiguous typed row
                    for (int j = 0; j < d; j++) {
                        const double oldx = row_get<T>(myrow, j);
                        row_set<T>(myrow, j, v[j * 64]);
                        v[j * 64] = oldx;
                    }
                    nll = mixture_eval<T>(p.ll, d, myrow);
                    nlp = mixture_eval<T>(p.lp, d, myrow);
                    nlq = mixture_eval<T>(p.lq, d, myrow);
                }
                const double lpn = log_p_t(nll, nlp, nlq, p.beta);
                const double lpo = log_p_t(oll, olp, olq, p.beta);
                const double log_a = (lpn + ref_corr(q1, p.nu, d)) - (lpo + ref_corr(q0, p.nu, d));
                const double u = accept_uniform(p.seed, gid, step);
                acc = log(u) < log_a;
                if (acc) {
                    ll[i] = nll;
                    lp[i] = nlp;
                    lq[i] = nlq;
                    n_acc++;
                } else {
                    for (int j = 0; j < d; j++) row_set<T>(myrow, j, v[j * 64]);  // restore old row
                }
            }
        }
        __syncthreads();
        if (active) {
            if (PHASE == 1) {
                tile_store<VEC>(reinterpret_cast<char*>(x_prop) + row0 * rowbytes, valid_bytes, rowbytes, ldsrow, tile, lane);
            } else {
                const unsigned long long accmask = __ballot(acc);
                if (accmask != 0ULL)
                    tile_store_rows<VEC>(reinterpret_cast<char*>(x) + row0 * rowbytes, valid_bytes, rowbytes, ldsrow, tile, lane, accmask);
            }
        }
        __syncthreads();
    }
    if (PHASE == 0) {
        __shared__ long long s_cnt[ASMC_BLOCK / 64];
        n_acc = wave_sum_ll(n_acc);
        if (lane == 0) s_cnt[wave] = n_acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            long long tsum = 0;
            for (int w = 0; w < (int)(blockDim.x >> 6); w++) tsum += s_cnt[w];
            block_counts[blockIdx.x] = tsum;
        }
    }
}

template <typename T, int D, int NOISE, int MODE>
__global__ __launch_bounds__(ASMC_BLOCK, 2) void k_pcn_reg(int64_t n, T* __restrict__ x, double* __restrict__ ll,
                                                          double* __restrict__ lp, double* __restrict__ lq,
                                                          const double* __restrict__ ptab, PcnScalars p,
                                                          const double* __restrict__ rho_ptr, uint32_t step,
                                                          long long* __restrict__ block_counts) {
    pcn_reg_body<T, D, NOISE, MODE>(n, x, ll, lp, lq, ptab, p, rho_ptr, step, block_counts);
}
// (a three-waves-per-SIMD build of the LDS-free step modes spills 200-300 B/lane to scratch and is slower: 0.19 vs 0.136 ms; round 6,
// with the blocked table: the pCN step at 168 registers spills 52 B and takes 165 us against 148 at two waves; the Student-t step
// fits three waves by itself - profiles/r06_ab_pcn_blocked_L.txt)

// Flow-proposal pCN on the whitened state, split around the flow's log-density kernel (asmc_flow.hip): the modes of
// k_pcn_reg_flow - PCN_FLOW_PROPOSE .. PCN_FLOW_PROPOSE_SXT_PROBIT - are listed and described in asmc_pcn_shared.h.
// packed table of the transform epilogue: TRTAB_ROWS rows of D doubles, then TRTAB_SCALARS scalars
//   rows: kind, lower, upper, mean, std, 1/(upper-lower), 1/std, premap a, b, lo, hi, h, q mean, q precision
//   scalars: eps, unit_logj, affine_logj, has_affine, q log-weight, has_q, minus_logj
// (TRTAB_ROWS, TRTAB_SCALARS: asmc_scratch.h, with the table's place in the context's scratch)

template <typename T, int D, int NOISE, int MODE>
__global__ __launch_bounds__(ASMC_BLOCK, 2) void k_pcn_reg_flow(
    int64_t n, T* __restrict__ y, T* __restrict__ x_prop, double* __restrict__ ll, double* __restrict__ lp,
    double* __restrict__ lq, double* __restrict__ ll_new, double* __restrict__ lp_new, const double* __restrict__ lq_new,
    const double* __restrict__ ptab, PcnScalars p, const double* __restrict__ rho_ptr, uint32_t step,
    long long* __restrict__ block_counts) {
    extern __shared__ __align__(16) char smem[];
    constexpr bool SOA = MODE >= PCN_FLOW_PROPOSE_S;
    constexpr bool TR = MODE == PCN_FLOW_PROPOSE_SXT_LOGIT || MODE == PCN_FLOW_PROPOSE_SXT_PROBIT;
    constexpr bool NO_DENS = MODE == PCN_FLOW_PROPOSE_SX || TR;
    constexpr bool HAS_LJ = MODE == PCN_FLOW_ACCEPT_SJ;
    constexpr int M = NO_DENS ? PCN_FLOW_PROPOSE : HAS_LJ ? PCN_FLOW_ACCEPT : SOA ? MODE - PCN_FLOW_PROPOSE_S : MODE;
    constexpr int ROWB = D * (int)sizeof(T);
    constexpr int LDSROW = ROWB + 16;
    const int WPB = (int)(blockDim.x >> 6);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    char* tile = smem + (size_t)wave * 64 * LDSROW;
    char* myrow = tile + lane * LDSROW;
    const double rho = *rho_ptr;
    const double a = sqrt(1.0 - rho * rho);
    long long n_acc = 0;
    const int64_t n_tiles = (n + 63) / 64;
    bm_d2* bmt = nullptr;  // Box-Muller tables of the default noise (see pcn_reg_body)
    if constexpr (NOISE == ASMC_NOISE_F64) {
        bmt = bm_lds();
        bm_tab_stage_rt(bmt, p.bmtab);
        __syncthreads();
    }
    const int64_t t = (int64_t)blockIdx.x * WPB + wave;  // one tile per wave, no loop (see k_pcn_reg)
    if (t < n_tiles) {
        const int64_t row0 = t * 64;
        const int64_t i = row0 + lane;
        const bool valid = i < n;
        const int64_t valid_bytes = ((n - row0) < 64 ? (n - row0) : 64) * (int64_t)ROWB;
        if (!SOA) tile_load<16>(reinterpret_cast<const char*>(y) + row0 * ROWB, valid_bytes, ROWB, LDSROW, tile, lane);
        // coordinate-major state through one buffer descriptor (see soa_load / soa_store)
        const unsigned long long ysa = (unsigned long long)(uintptr_t)p.ys;
        T* ysu = reinterpret_cast<T*>(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(ysa >> 32)) << 32) |
                                      (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)ysa));
        const __amdgpu_buffer_rsrc_t ysr = __builtin_amdgcn_make_buffer_rsrc(
            ysu, 0, SOA ? (int)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)p.n_pad * D * sizeof(T))) : 0,
            0x00020000);
        const unsigned ys_tile = (unsigned)__builtin_amdgcn_readfirstlane((int)t) * 64u * (unsigned)sizeof(T);
        const unsigned ys_row = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)p.n_pad) * (unsigned)sizeof(T);
        const unsigned ys_lane = (unsigned)lane * (unsigned)sizeof(T);
        double oll = 0.0, olp = 0.0, olq = 0.0, nll = 0.0, nlp = 0.0, nlq = 0.0;
        double olj = 0.0, nlj = 0.0;
        double* const lj = HAS_LJ ? static_cast<double*>(static_cast<void*>(y)) : nullptr;
        if (valid && M == PCN_FLOW_ACCEPT) {
            oll = ll[i], olp = lp[i], olq = lq[i];
            nll = ll_new[i], nlp = lp_new[i], nlq = lq_new[i];
            if (HAS_LJ) olj = lj[i], nlj = static_cast<const double*>(static_cast<const void*>(x_prop))[i];
        }
        wave_lds_sync();
        bool acc = false;
        const double* __restrict__ Lp = ptab;
        const double* __restrict__ mup = ptab + 2 * PTAB_TRI(D);
        const double* __restrict__ m0 = ptab + 2 * PTAB_TRI(D) + D;
        const MixDev mll = {p.c_ll, m0, m0 + ASMC_MAX_COMPONENTS, m0 + ASMC_MAX_COMPONENTS * (1 + D)};
        const MixDev mlp = {p.c_lp, m0 + PTAB_MIX(D), m0 + PTAB_MIX(D) + ASMC_MAX_COMPONENTS,
                            m0 + PTAB_MIX(D) + ASMC_MAX_COMPONENTS * (1 + D)};
        if (valid) {
            const unsigned long long gid = p.gid0 + (unsigned long long)i;
            double v[D];
            if (SOA) {
#pragma unroll
                for (int j = 0; j < D; j++) v[j] = soa_load<T>(ysr, ys_lane, ys_tile + (unsigned)j * ys_row);
            } else {
                row_to_regs<T, D>(myrow, v);
            }
            double q0 = 0.0, q1 = 0.0;
#pragma unroll
            for (int j = 0; j < D; j++) q0 = fma(v[j], v[j], q0);
            const double rs = tpcn_scale(rho, p.nu, q0, p.gam, i);  // the same variate in both modes
            if (NOISE == ASMC_NOISE_F64) {
#pragma unroll
                for (int qd = 0; qd < (D + 3) / 4; qd++) {
                    double z[4];
                    normal_quad(p.seed, gid, step, (uint32_t)qd, bmt, z[0], z[1], z[2], z[3]);
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        if (4 * qd + e < D) {
                            v[4 * qd + e] = (double)(T)fma(rs, z[e], a * v[4 * qd + e]);
                            q1 = fma(v[4 * qd + e], v[4 * qd + e], q1);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else {
#pragma unroll
                for (int qd = 0; qd < D / 4; qd++) {
                    double z[4];
                    normal_quad_f32(p.seed, gid, step, (uint32_t)qd, z[0], z[1], z[2], z[3]);
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        v[4 * qd + e] = (double)(T)fma(rs, z[e], a * v[4 * qd + e]);
                        q1 = fma(v[4 * qd + e], v[4 * qd + e], q1);
                    }
                    if (qd & 1) __builtin_amdgcn_sched_barrier(0);
                }
            }
            if (M == PCN_FLOW_PROPOSE) {
                tri_matvec_inplace<D>(Lp, v);
#pragma unroll
                for (int j = 0; j < D; j++) v[j] = (double)(T)(mup[j] + v[j]);
                if (!NO_DENS) {
                    ll_new[i] = mixture_eval_regs<D>(mll, v);
                    lp_new[i] = mixture_eval_regs<D>(mlp, v);
                }
                if (TR) {
                    constexpr int HINTS = ASMC_TR_NO_PERIODIC |
                                          (MODE == PCN_FLOW_PROPOSE_SXT_LOGIT ? ASMC_TR_NO_PROBIT : ASMC_TR_NO_LOGIT);
                    const double* __restrict__ tt = lq_new;
                    const double* __restrict__ sc = tt + TRTAB_ROWS * D;
                    const double eps = sc[0];
                    const bool has_affine = sc[3] != 0.0, has_q = sc[5] != 0.0;
                    double lj_b = 0.0, quad = 0.0, qq = 0.0;
                    bool any_b = false;
#pragma unroll
                    for (int j = 0; j < D; j++) {
                        if (has_q) {  // log q(x') from z' (asmc_mixture_logpdf_premap)
                            const double tq = clip(v[j] * tt[7 * D + j] + tt[8 * D + j], tt[9 * D + j], tt[10 * D + j]);
                            quad = fma(tt[11 * D + j] * tq, tq, quad);
                            const double dq = tq - tt[12 * D + j];
                            qq = fma(dq * dq, tt[13 * D + j], qq);
                        }
                        CoordPar c;
                        c.kind = (int)tt[j], c.periodic = 0;
                        c.lo = tt[D + j], c.up = tt[2 * D + j], c.mean = tt[3 * D + j], c.std = tt[4 * D + j];
                        c.inv_w = tt[5 * D + j], c.inv_std = tt[6 * D + j];
                        any_b |= c.kind != 0;
                        v[j] = (double)(T)transform_coord<1, HINTS>(v[j], c, has_affine, eps, lj_b);
                        // keep the table reads of later coordinates behind this one's arithmetic (hoisted, they cost 100 VGPRs)
                        if ((j & 1) == 1) __builtin_amdgcn_sched_barrier(0);
                    }
                    double lj = 0.0;  // k_transform's grouping: affine constant, then the bounded block
                    if (has_affine) lj += -sc[2];
                    if (any_b) lj += lj_b + (-sc[1]);
                    ll_new[i] = lj;
                    if (has_q) lp_new[i] = ((sc[4] - 0.5 * qq) + quad) - (sc[6] != 0.0 ? lj : 0.0);
                }
                regs_to_row<T, D>(myrow, v);
                acc = true;
            } else {
                double lpn = log_p_t(nll, nlp, nlq, p.beta);
                double lpo = log_p_t(oll, olp, olq, p.beta);
                if (HAS_LJ) {  // as k_pcn_accept_flags: the log-Jacobian joins the tempered log-target, NaN -> -inf
                    lpn += nlj, lpo += olj;
                    lpn = log_p_t_guard(lpn);
                    lpo = log_p_t_guard(lpo);
                }
                const double log_a = (lpn + ref_corr(q1, p.nu, D)) - (lpo + ref_corr(q0, p.nu, D));
                const double u = accept_uniform(p.seed, gid, step);
                acc = log(u) < log_a;
                if (acc) {
                    if (HAS_LJ) lj[i] = nlj;
                    if (SOA) {
#pragma unroll
                        for (int j = 0; j < D; j++) soa_store<T>(ysr, ys_lane, ys_tile + (unsigned)j * ys_row, v[j]);
                    } else {
                        regs_to_row<T, D>(myrow, v);
                    }
                    ll[i] = nll;
                    lp[i] = nlp;
                    lq[i] = nlq;
                    n_acc++;
                }
            }
        }
        wave_lds_sync();
        {
            const unsigned long long accmask = (SOA && M == PCN_FLOW_ACCEPT) ? 0ULL : __ballot(acc);
            char* obase = reinterpret_cast<char*>(M == PCN_FLOW_PROPOSE ? x_prop : y) + row0 * ROWB;
            if (accmask != 0ULL) tile_store_rows<16>(obase, valid_bytes, ROWB, LDSROW, tile, lane, accmask);
        }
        wave_lds_sync();
    }
    if (M == PCN_FLOW_ACCEPT) {
        __shared__ long long s_cnt[ASMC_BLOCK / 64];
        n_acc = wave_sum_ll(n_acc);
        if (lane == 0) s_cnt[wave] = n_acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            long long tsum = 0;
            for (int w = 0; w < WPB; w++) tsum += s_cnt[w];
            block_counts[blockIdx.x] = tsum;
        }
    }
}

// tpCN: unit-scale Gamma(shape) variates of every particle for the Markov steps step .. step + nsteps - 1 (Marsaglia-Tsang,
// counter based: a step's variates do not depend on the chain, so several steps are drawn by one launch)
template <bool F32>
__global__ __launch_bounds__(ASMC_BLOCK) void k_gamma_draw(int64_t n, double shape, unsigned long long seed,
                                                          unsigned long long gid0, uint32_t step, int nsteps, int64_t stride_n,
                                                          double* __restrict__ out, const double* __restrict__ bmtab) {
    bm_d2* bmt = nullptr;
    if constexpr (!F32) {
        bmt = bm_lds();
        bm_tab_stage<ASMC_BLOCK>(bmt, bmtab);
        __syncthreads();
    }
    const int64_t stride = (int64_t)gridDim.x * ASMC_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x; i < n; i += stride)
        for (int s = 0; s < nsteps; s++)
            out[(size_t)s * stride_n + i] = gamma_unit<F32>(shape, seed, gid0 + (unsigned long long)i, step + (uint32_t)s, bmt);
}

// before a step kernel: points pd.gam at the step's scale variates in ctx->d_gamma (tpCN only), drawing the next
// ASMC_GAMMA_BATCH steps' worth when the step is not among those already there (one launch per eight steps instead of one
// per step: 15 us of every 150 us step)
int pcn_prepare_gamma(asmc_ctx* ctx, int64_t n, PcnDev& pd, uint32_t step, hipStream_t st) {
    if (!(pd.nu > 0.0)) {
        pd.gam = nullptr;
        return ASMC_OK;
    }
    const double shape = 0.5 * ((double)(pd.d_noise > 0 ? pd.d_noise : pd.d) + pd.nu);
    const int64_t stride_n = (n + 63) / 64 * 64;
    const bool hit = ctx->gam_count > 0 && ctx->gam_n == n && ctx->gam_seed == (unsigned long long)pd.seed &&
                     ctx->gam_gid0 == (unsigned long long)pd.gid0 && ctx->gam_shape == shape && ctx->gam_noise == pd.noise &&
                     step >= ctx->gam_step0 && step - ctx->gam_step0 < (uint32_t)ctx->gam_count;
    if (!hit) {
        int batch = (int)((int64_t)ASMC_GAMMA_BATCH * ctx->n_max / stride_n);  // what the buffer holds
        if (batch > ASMC_GAMMA_BATCH) batch = ASMC_GAMMA_BATCH;
        if (batch < 1) batch = 1;
        static const bool single = getenv("ASMC_GAMMA_PER_STEP") != nullptr;
        if (single) batch = 1;
        const int grid = grid_for(n, ASMC_BLOCK, ASMC_MAX_BLOCKS * 4);
        if (pd.noise == ASMC_NOISE_F32)
            ASMC_LAUNCH(ctx, st, "k_gamma_draw", k_gamma_draw<true>, dim3(grid), dim3(ASMC_BLOCK), 0, st, n, shape,
                        (unsigned long long)pd.seed, (unsigned long long)pd.gid0, step, batch, stride_n, ctx->d_gamma,
                        (const double*)ctx->d_bmtab);
        else
            ASMC_LAUNCH(ctx, st, "k_gamma_draw", k_gamma_draw<false>, dim3(grid), dim3(ASMC_BLOCK), 0, st, n, shape,
                        (unsigned long long)pd.seed, (unsigned long long)pd.gid0, step, batch, stride_n, ctx->d_gamma,
                        (const double*)ctx->d_bmtab);
        ASMC_LAUNCH_CHECK();
        ctx->gam_n = n, ctx->gam_seed = (unsigned long long)pd.seed, ctx->gam_gid0 = (unsigned long long)pd.gid0;
        ctx->gam_shape = shape, ctx->gam_noise = pd.noise, ctx->gam_step0 = step, ctx->gam_count = batch;
    }
    pd.gam = ctx->d_gamma + (size_t)(step - ctx->gam_step0) * stride_n;
    return ASMC_OK;
}

// sums the per-block accept counts of step `t`, records them, adapts the step size
// (log rho += (acc - target)/(t+1)^0.75, rho clipped to [1e-4, 0.99])
// adapt: 0 = off, 1 = after every step, k >= 2 = LAGGED (sampler_kwargs["adapt_lag"] = k): the step size is held for blocks of k
// steps; the step that ends a block (t + 1 = 0 mod k, or `last`: the final step of the call) applies the block's updates in
// order, each with its own count and step index - the same arithmetic k steps late.  A sharded run then exchanges its accept
// counts once per block (k cells in one all-reduce) instead of once per step.
// cells != NULL (sharded, lagged): block_counts is unused; the GLOBAL counts of the block's steps sit in cells[t' % k] and are
// recorded here (counts_out, rho_hist) together with the replay.
__global__ __launch_bounds__(1024) void k_pcn_adapt(int nblocks, const long long* __restrict__ block_counts,
                                                   int64_t n, int t, long long* __restrict__ counts_out,
                                                   double* __restrict__ rho_ptr, double* __restrict__ rho_hist,
                                                   double target, int adapt, const double* __restrict__ rho_src, int last,
                                                   const long long* __restrict__ cells) {
    // rho_src: where the step size step t used is kept when it is not *rho_ptr (fused flow steps of sharded runs, which
    // adapt in the next step's prologue: *rho_ptr is only brought up to date here, at the end of a call)
    __shared__ long long s_c[16];
    long long c = 0;
    if (cells == nullptr)
        for (int b = threadIdx.x; b < nblocks; b += 1024) c += block_counts[b];
    c = wave_sum_ll(c);
    if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        c = 0;
        for (int w = 0; w < 16; w++) c += s_c[w];
        const double rho = rho_src ? *rho_src : *rho_ptr;
        if (cells == nullptr) {
            counts_out[t] = c;
            rho_hist[t] = rho;
        }
        if (adapt <= 1) {
            *rho_ptr = adapt ? pcn_adapt_rho(rho, c, n, target, t) : rho;
        } else if ((t + 1) % adapt == 0 || last) {
            double r = rho;
            for (int tp = t - (t % adapt); tp <= t; tp++) {
                const long long ct = cells ? cells[tp % adapt] : (tp == t ? c : counts_out[tp]);
                if (cells) counts_out[tp] = ct, rho_hist[tp] = rho;
                r = pcn_adapt_rho(r, ct, n, target, tp);
            }
            *rho_ptr = r;
        } else {
            *rho_ptr = rho;
        }
    }
}

__global__ void k_set_scalar(double* __restrict__ cell, double v) { *cell = v; }

__global__ __launch_bounds__(1024) void k_count_sum(int nblocks, const long long* __restrict__ block_counts,
                                                   long long* __restrict__ cell) {  // (the caller points `cell` at the step's own cell)
    __shared__ long long s_c[16];
    long long c = 0;
    for (int b = threadIdx.x; b < nblocks; b += 1024) c += block_counts[b];
    c = wave_sum_ll(c);
    if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        c = 0;
        for (int w = 0; w < 16; w++) c += s_c[w];
        cell[0] = c;
    }
}

// closes step t: accept count (summed across ranks through the exchange hook when one is installed), history, adaptation.
// `last`: t is the final step of the call (a lagged adaptation closes its open block there).
int pcn_close_step(asmc_ctx* ctx, hipStream_t st, int grid, const long long* d_block, int64_t n, int t, long long* d_counts,
                   double* d_rho, double* d_rho_hist, double target, int adapt, int last) {
    if (ctx->count_hook) {
        const int lag = adapt >= 2 ? adapt : 1;
        if (lag > ctx->count_cells) {
            asmc_set_error("adapt_lag %d needs %d exchange cells, the installed hook has %d (asmc_pcn_set_count_cells)", lag, lag, ctx->count_cells);
            return ASMC_ERR_ARG;
        }
        ASMC_LAUNCH(ctx, st, "k_count_sum", k_count_sum, dim3(1), dim3(1024), 0, st, grid, d_block, ctx->count_cell + (lag > 1 ? t % lag : 0));
        ASMC_LAUNCH_CHECK();
        if (lag > 1 && !((t + 1) % lag == 0 || last)) return ASMC_OK;  // the block's counts are exchanged together, at its end
        const int hrc = ctx->count_hook(ctx->count_hook_user, reinterpret_cast<asmc_stream>(st));
        if (hrc != 0) {
            asmc_set_error("accept-count exchange hook failed (%d)", hrc);
            return ASMC_ERR_ARG;
        }
        ASMC_LAUNCH(ctx, st, "k_pcn_adapt", k_pcn_adapt, dim3(1), dim3(1024), 0, st, 1, (const long long*)ctx->count_cell,
                    ctx->count_n_global, t, d_counts, d_rho, d_rho_hist, target, adapt, (const double*)nullptr, last,
                    lag > 1 ? (const long long*)ctx->count_cell : (const long long*)nullptr);
    } else {
        ASMC_LAUNCH(ctx, st, "k_pcn_adapt", k_pcn_adapt, dim3(1), dim3(1024), 0, st, grid, d_block, n, t, d_counts, d_rho,
                    d_rho_hist, target, adapt, (const double*)nullptr, last, (const long long*)nullptr);
    }
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

// split-path accept: per particle decision + scalar update, then a flat conditional row copy
__global__ __launch_bounds__(ASMC_BLOCK) void k_pcn_accept_flags(
    int64_t n, double* __restrict__ ll, double* __restrict__ lp, double* __restrict__ lq,
    const double* __restrict__ ll_new, const double* __restrict__ lp_new, const double* __restrict__ lq_new,
    double* __restrict__ lj_old, const double* __restrict__ lj_new, const double* __restrict__ qf_old,
    const double* __restrict__ qf_new, double beta, unsigned long long seed, unsigned long long gid0,
    uint32_t step, unsigned char* __restrict__ flags, unsigned long long* __restrict__ count) {
    long long c = 0;
    const int64_t stride = (int64_t)gridDim.x * ASMC_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x; i < n; i += stride) {
        double lpn = log_p_t(ll_new[i], lp_new[i], lq_new[i], beta);
        double lpo = log_p_t(ll[i], lp[i], lq[i], beta);
        if (lj_new) {
            lpn += lj_new[i];
            lpn = log_p_t_guard(lpn);
        }
        if (lj_old) {
            lpo += lj_old[i];
            lpo = log_p_t_guard(lpo);
        }
        const double log_a = (lpn + 0.5 * qf_new[i]) - (lpo + 0.5 * qf_old[i]);
        const double u = accept_uniform(seed, gid0 + (unsigned long long)i, step);
        const bool acc = log(u) < log_a;
        flags[i] = acc ? 1 : 0;
        if (acc) {
            ll[i] = ll_new[i];
            lp[i] = lp_new[i];
            lq[i] = lq_new[i];
            if (lj_old && lj_new) lj_old[i] = lj_new[i];  // the carried log-Jacobian follows the accepted state
            c++;
        }
    }
    // one atomic per block (thousands of same-address atomics serialise at the L2: 8192 per-wave adds cost ~80 us)
    __shared__ long long s_c[ASMC_BLOCK / 64];
    c = wave_sum_ll(c);
    if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t = 0;
        for (int w = 0; w < ASMC_BLOCK / 64; w++) t += s_c[w];
        if (t) atomicAdd(count, (unsigned long long)t);
    }
}

template <typename T>
__global__ __launch_bounds__(ASMC_BLOCK) void k_copy_flagged_rows(int64_t n, int d, T* __restrict__ x,
                                                                 const T* __restrict__ x_prop,
                                                                 const unsigned char* __restrict__ flags) {
    const int64_t total = n * d;
    const int64_t stride = (int64_t)gridDim.x * ASMC_BLOCK;
    for (int64_t e = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x; e < total; e += stride) {
        const int64_t r = e / d;
        if (flags[r]) x[e] = x_prop[e];
    }
}

// the same in 16-byte pieces, `cpr` pieces per row (row bytes a multiple of 16, n * cpr < 2^32): the row index comes from
// a multiplication with magic = floor(2^32 / cpr) + 1 instead of a 64-bit division per element
__global__ __launch_bounds__(ASMC_BLOCK) void k_copy_flagged_rows16(unsigned total, int shift, unsigned magic,
                                                                   uint4* __restrict__ x, const uint4* __restrict__ x_prop,
                                                                   const unsigned char* __restrict__ flags) {
    const unsigned stride = gridDim.x * ASMC_BLOCK;
    for (unsigned e = blockIdx.x * ASMC_BLOCK + threadIdx.x; e < total; e += stride) {
        const unsigned r = shift >= 0 ? e >> shift : (unsigned)(((unsigned long long)e * magic) >> 32);
        if (flags[r]) x[e] = x_prop[e];
    }
}

int launch_copy_flagged(asmc_ctx* ctx, int64_t n, int d, int x_dtype, void* x, const void* x_prop, const unsigned char* flags,
                        hipStream_t st) {
    const int64_t rowb = (int64_t)d * (x_dtype == ASMC_F64 ? 8 : 4);
    const int64_t cpr = rowb / 16;
    // power-of-two piece counts shift; otherwise e * (floor(2^32 / cpr) + 1) >> 32 == e / cpr, exact while e * cpr < 2^32
    const bool pow2 = cpr > 0 && (cpr & (cpr - 1)) == 0;
    int shift = -1;
    if (pow2)
        for (shift = 0; (1LL << shift) < cpr; shift++) {
        }
    if (rowb % 16 == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)x_prop % 16) == 0 && n * cpr < (1LL << 32) &&
        (pow2 || n * cpr * cpr < (1LL << 32))) {
        const unsigned total = (unsigned)(n * cpr);
        const int grid = grid_for(total, ASMC_BLOCK * 4, ASMC_MAX_BLOCKS * 4);
        ASMC_LAUNCH(ctx, st, "k_copy_flagged_rows", k_copy_flagged_rows16, dim3(grid), dim3(ASMC_BLOCK), 0, st, total, shift,
                    (unsigned)(0xFFFFFFFFu / (unsigned)cpr + 1u), (uint4*)x, (const uint4*)x_prop, flags);
    } else {
        const int grid2 = grid_for(n * d, ASMC_BLOCK * 4, ASMC_MAX_BLOCKS * 2);
        if (x_dtype == ASMC_F64)
            ASMC_LAUNCH(ctx, st, "k_copy_flagged_rows<double>", k_copy_flagged_rows<double>, dim3(grid2), dim3(ASMC_BLOCK), 0, st, n, d,
                        (double*)x, (const double*)x_prop, flags);
        else
            ASMC_LAUNCH(ctx, st, "k_copy_flagged_rows<float>", k_copy_flagged_rows<float>, dim3(grid2), dim3(ASMC_BLOCK), 0, st, n, d,
                        (float*)x, (const float*)x_prop, flags);
    }
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

// =============================================================================================
// host side
// =============================================================================================
// gather the caller's tables into the ctx parameter block (one tiny kernel, stream ordered)
__global__ __launch_bounds__(256) void k_pcn_pack(PcnDev pd, double* __restrict__ t, double* __restrict__ rho_cell, double rho) {
    if (rho_cell && threadIdx.x == 0) *rho_cell = rho;  // (the call's starting step size rides along: no k_set_scalar launch)
    pcn_pack_block(pd, t);
}

int pack_pcn_tables(asmc_ctx* ctx, const PcnDev& pd, hipStream_t st, double* rho_cell, double rho) {
    ctx->ptab_tag = 0;
    ASMC_LAUNCH(ctx, st, "k_pcn_pack", k_pcn_pack, dim3(1), dim3(256), 0, st, pd, ctx->d_ptab, rho_cell, rho);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

bool pcn_reg_supported(int d, size_t elem, const void* x) {
    return (d == 4 || d == 8 || d == 16 || d == 32) && (d * elem) % 16 == 0 && ((uintptr_t)x % 16) == 0 &&
           !pcn_env_generic();
}

// the by-value part of a launch's parameters (the tables travel in ctx->d_ptab)
static PcnScalars pcn_scalars(const PcnDev& pd) {
    PcnScalars ps;
    ps.beta = pd.beta;
    ps.nu = pd.nu;
    ps.gam = pd.gam;
    ps.ys = pd.ys;
    ps.n_pad = pd.n_pad;
    ps.d_real = pd.d;
    ps.seed = pd.seed;
    ps.gid0 = pd.gid0;
    ps.bmtab = pd.bmtab;
    ps.tile_par = pd.tile_par;
    ps.d_noise = pd.d_noise;
    ps.c_ll = pd.ll.C;
    ps.c_lp = pd.lp.C;
    ps.c_lq = pd.lq.C;
    return ps;
}

// the profile label of k_pcn_reg's modes
static constexpr const char* pcn_reg_label(int mode) {
    return mode == PCN_X_STEP ? "k_pcn_reg"
           : (mode == PCN_Y_STEP || mode == PCN_Y_STEP_S || mode == PCN_Y_STEP_SG) ? "k_pcn_reg_y"
           : mode == PCN_X_STEP_T ? "k_tpcn_reg"
           : (mode == PCN_Y_STEP_T || mode == PCN_Y_STEP_TS || mode == PCN_Y_STEP_TSG) ? "k_tpcn_reg_y"
           : (mode == PCN_WHITEN || mode == PCN_WHITEN_S) ? "k_pcn_whiten"
           : (mode >= PCN_X_PROPOSE && mode <= PCN_X_PROPOSE_PAD_T) ? "k_pcn_propose_reg"
                                                                    : "k_pcn_unwhiten";
}

template <typename T, int D, int NOISE, int MODE>
static int launch_pcn_reg(asmc_ctx* ctx, int64_t n, T* x, double* ll, double* lp, double* lq, const PcnDev& pd,
                          const double* rho_ptr, uint32_t step, long long* block_counts, int* grid_out, hipStream_t st) {
    constexpr int LDSROW = D * (int)sizeof(T) + 16;
    // waves per block: 160 KB of LDS hold floor(160K / tile) wave tiles; blocks of 4 waves waste the remainder
    // when the tile is large (d = 32 fp64: 17 KB tiles -> 2 blocks of 4 = 8 waves, but 9 single-wave blocks)
    constexpr size_t tile_bytes = (size_t)64 * LDSROW;
    static int wpb_env = getenv("ASMC_PCN_WPB") ? atoi(getenv("ASMC_PCN_WPB")) : 0;
    constexpr bool NO_LDS = MODE == PCN_Y_STEP_S || MODE == PCN_Y_STEP_TS || MODE == PCN_Y_STEP_SG ||
                            MODE == PCN_Y_STEP_TSG;  // coordinate-major state: registers only
    // kernels that draw the default noise keep its 6 KB of tables per BLOCK next to the tiles: four waves share them
    constexpr bool BM = NOISE == ASMC_NOISE_F64 && !(MODE == PCN_WHITEN || MODE == PCN_WHITEN_S || MODE == PCN_UNWHITEN ||
                                                     MODE == PCN_UNWHITEN_S || MODE == PCN_UNWHITEN_X || MODE == PCN_UNWHITEN_XS);
    const int wpb = wpb_env > 0 ? wpb_env : (BM || NO_LDS || (160 * 1024) / tile_bytes % 4 == 0 || tile_bytes * 12 <= 160 * 1024 ? 4 : 1);
    const size_t lds_bytes = NO_LDS ? 0 : (size_t)wpb * tile_bytes;
    const int64_t n_tiles = (n + 63) / 64;
    const int64_t grid64 = (n_tiles + wpb - 1) / wpb;
    if (grid64 > ASMC_PCN_MAX_GRID) {
        asmc_set_error("pcn: n=%lld exceeds the per-call block budget", (long long)n);
        return ASMC_ERR_UNSUPPORTED;
    }
    const int grid = (int)grid64;
    *grid_out = grid;
    auto kern = k_pcn_reg<T, D, NOISE, MODE>;
    static bool attr_set_dev[ASMC_MAX_DEVICES] = {false}; bool& attr_set = attr_set_dev[asmc_dev_slot(ctx)];  // per instantiation; the attribute call costs tens of microseconds
    if (lds_bytes > 64 * 1024 && !attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        attr_set = true;
    }
    const PcnScalars ps = pcn_scalars(pd);
    ASMC_LAUNCH(ctx, st, pcn_reg_label(MODE), kern, dim3(grid), dim3(wpb * 64), lds_bytes, st, n, x, ll, lp, lq,
                (const double*)ctx->d_ptab, ps, rho_ptr, step, block_counts);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

template <typename T, int D, int NOISE, int MODE>
static int launch_pcn_reg_flow(asmc_ctx* ctx, int64_t n, T* y, T* x_prop, double* ll, double* lp, double* lq,
                               double* ll_new, double* lp_new, const double* lq_new, const PcnDev& pd,
                               const double* rho_ptr, uint32_t step, long long* block_counts, int* grid_out,
                               hipStream_t st) {
    constexpr int LDSROW = D * (int)sizeof(T) + 16;
    constexpr size_t tile_bytes = (size_t)64 * LDSROW;
    constexpr bool NO_LDS = MODE == PCN_FLOW_ACCEPT_S || MODE == PCN_FLOW_ACCEPT_SJ;
    const int wpb = (NOISE == ASMC_NOISE_F64 || NO_LDS || (160 * 1024) / tile_bytes % 4 == 0 || tile_bytes * 12 <= 160 * 1024) ? 4 : 1;  // (f64 noise: 6 KB of tables per block)
    const size_t lds_bytes = NO_LDS ? 0 : (size_t)wpb * tile_bytes;
    const int64_t grid64 = ((n + 63) / 64 + wpb - 1) / wpb;
    if (grid64 > ASMC_PCN_MAX_GRID) {
        asmc_set_error("pcn: n=%lld exceeds the per-call block budget", (long long)n);
        return ASMC_ERR_UNSUPPORTED;
    }
    *grid_out = (int)grid64;
    auto kern = k_pcn_reg_flow<T, D, NOISE, MODE>;
    static bool attr_set_dev[ASMC_MAX_DEVICES] = {false}; bool& attr_set = attr_set_dev[asmc_dev_slot(ctx)];
    if (lds_bytes > 64 * 1024 && !attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        attr_set = true;
    }
    const PcnScalars ps = pcn_scalars(pd);
    ASMC_LAUNCH(ctx, st, (MODE == PCN_FLOW_PROPOSE || MODE == PCN_FLOW_PROPOSE_S || MODE == PCN_FLOW_PROPOSE_SX || MODE >= PCN_FLOW_PROPOSE_SXT_LOGIT) ? "k_pcn_flow_propose" : "k_pcn_flow_accept", kern, dim3((int)grid64),
                dim3(wpb * 64), lds_bytes, st, n, y, x_prop, ll, lp, lq, ll_new, lp_new, lq_new, (const double*)ctx->d_ptab, ps,
                rho_ptr, step, block_counts);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

template <typename T, int MODE>
static int dispatch_pcn_reg_flow(asmc_ctx* ctx, int64_t n, T* y, T* x_prop, double* ll, double* lp, double* lq,
                                 double* ll_new, double* lp_new, const double* lq_new, const PcnDev& pd,
                                 const double* rho_ptr, uint32_t step, long long* block_counts, int* grid_out,
                                 hipStream_t st) {
#define PCN_FLOW_CASE(DD)                                                                                              \
    if (pd.d == DD) {                                                                                                  \
        if (pd.noise == ASMC_NOISE_F32)                                                                                \
            return launch_pcn_reg_flow<T, DD, ASMC_NOISE_F32, MODE>(ctx, n, y, x_prop, ll, lp, lq, ll_new, lp_new, lq_new, \
                                                                    pd, rho_ptr, step, block_counts, grid_out, st);   \
        return launch_pcn_reg_flow<T, DD, ASMC_NOISE_F64, MODE>(ctx, n, y, x_prop, ll, lp, lq, ll_new, lp_new, lq_new, pd, \
                                                                rho_ptr, step, block_counts, grid_out, st);           \
    }
    PCN_FLOW_CASE(4)
    PCN_FLOW_CASE(8)
    PCN_FLOW_CASE(16)
    PCN_FLOW_CASE(32)
#undef PCN_FLOW_CASE
    asmc_set_error("pcn flow: d=%d has no register-resident kernel", pd.d);
    return ASMC_ERR_UNSUPPORTED;
}

// LDS of one wave of the generic kernel: its 64-row tile and the 64 x d work vectors.  Widths that have no other kernel
// (d > 128) are checked against the budget by the entry points, before anything is launched.
static size_t pcn_generic_wave_bytes(int d, size_t elem) { return (size_t)64 * lds_row_stride(d * (int)elem) + (size_t)64 * 8 * d; }
static bool pcn_generic_fits(int d, size_t elem) { return pcn_generic_wave_bytes(d, elem) <= 160 * 1024 - 1024 - BM_TAB_N * 16; }
int pcn_generic_check(int d, int x_dtype) {
    const size_t elem = x_dtype == ASMC_F64 ? 8 : 4;
    if (d > 128 && !pcn_generic_fits(d, elem)) {
        asmc_set_error("pcn: d=%d needs %zu B of LDS per wave (unsupported)", d, pcn_generic_wave_bytes(d, elem));
        return ASMC_ERR_UNSUPPORTED;
    }
    return ASMC_OK;
}

template <typename T, int PHASE>
static int launch_pcn_step(asmc_ctx* ctx, int64_t n, T* x, double* ll, double* lp, double* lq, const PcnDev& pd,
                           const double* rho_ptr, uint32_t step, long long* block_counts, int* grid_out,
                           T* x_prop, double* qf_old, double* qf_new, hipStream_t st) {
    const int rowbytes = pd.d * (int)sizeof(T);
    if (PHASE == 0 && (pd.dpad > pd.d || pcn_reg_supported(pd.d, sizeof(T), x))) {
        const int dk = pd.dpad > pd.d ? pd.dpad : pd.d;
        switch (dk * 64 + (pd.noise == ASMC_NOISE_F32 ? 32 : 0) + pd.mode) {  // register-resident specialisations
#define PCN_CASE2(DD, NZ, MD) \
    case DD * 64 + (NZ == ASMC_NOISE_F32 ? 32 : 0) + MD: \
        return launch_pcn_reg<T, DD, NZ, MD>(ctx, n, x, ll, lp, lq, pd, rho_ptr, step, block_counts, grid_out, st);
#define PCN_CASE(DD)                            \
    PCN_CASE2(DD, ASMC_NOISE_F64, PCN_X_STEP)   \
    PCN_CASE2(DD, ASMC_NOISE_F32, PCN_X_STEP)   \
    PCN_CASE2(DD, ASMC_NOISE_F64, PCN_Y_STEP)   \
    PCN_CASE2(DD, ASMC_NOISE_F32, PCN_Y_STEP)   \
    PCN_CASE2(DD, ASMC_NOISE_F64, PCN_X_STEP_T) \
    PCN_CASE2(DD, ASMC_NOISE_F32, PCN_X_STEP_T) \
    PCN_CASE2(DD, ASMC_NOISE_F64, PCN_Y_STEP_T) \
    PCN_CASE2(DD, ASMC_NOISE_F32, PCN_Y_STEP_T) \
    PCN_CASE2(DD, ASMC_NOISE_F64, PCN_Y_STEP_S)  \
    PCN_CASE2(DD, ASMC_NOISE_F32, PCN_Y_STEP_S)  \
    PCN_CASE2(DD, ASMC_NOISE_F64, PCN_Y_STEP_TS) \
    PCN_CASE2(DD, ASMC_NOISE_F32, PCN_Y_STEP_TS) \
    PCN_CASE2(DD, ASMC_NOISE_F64, PCN_Y_STEP_SG)  \
    PCN_CASE2(DD, ASMC_NOISE_F32, PCN_Y_STEP_SG)  \
    PCN_CASE2(DD, ASMC_NOISE_F64, PCN_Y_STEP_TSG) \
    PCN_CASE2(DD, ASMC_NOISE_F32, PCN_Y_STEP_TSG) \
    PCN_CASE2(DD, ASMC_NOISE_F64, PCN_WHITEN_S)  \
    PCN_CASE2(DD, ASMC_NOISE_F64, PCN_UNWHITEN_S) \
    PCN_CASE2(DD, ASMC_NOISE_F64, PCN_UNWHITEN_XS) \
    PCN_CASE2(DD, ASMC_NOISE_F64, PCN_X_PROPOSE) \
    PCN_CASE2(DD, ASMC_NOISE_F64, PCN_X_PROPOSE_T) \
    PCN_CASE2(DD, ASMC_NOISE_F64, PCN_WHITEN)   \
    PCN_CASE2(DD, ASMC_NOISE_F64, PCN_UNWHITEN) \
    PCN_CASE2(DD, ASMC_NOISE_F64, PCN_UNWHITEN_X)
#ifdef PCN_DIAG_ONLY_D32S  // diagnostic builds (generated-code experiments): the coordinate-major d = 32 steps alone
            PCN_CASE2(32, ASMC_NOISE_F64, PCN_Y_STEP_S)
            PCN_CASE2(32, ASMC_NOISE_F64, PCN_Y_STEP_TS)
#else
            PCN_CASE(4)
            PCN_CASE(8)
            PCN_CASE(16)
            PCN_CASE(32)
            PCN_CASE2(32, ASMC_NOISE_F64, PCN_X_PROPOSE_PAD)
            PCN_CASE2(32, ASMC_NOISE_F64, PCN_X_PROPOSE_PAD_T)
#endif
#undef PCN_CASE
#undef PCN_CASE2
            default: break;
        }
    }
    if (pd.mode >= PCN_WHITEN_S) {  // coordinate-major / propose modes exist as register kernels only
        asmc_set_error("pcn: no kernel for mode %d at d=%d, noise=%d", pd.mode, pd.d, pd.noise);
        return ASMC_ERR_UNSUPPORTED;
    }
    const size_t per_wave = pcn_generic_wave_bytes(pd.d, sizeof(T));
    size_t lds_bytes = 0;
    const int wpb = waves_for_lds(per_wave, &lds_bytes);
    if (!pcn_generic_fits(pd.d, sizeof(T))) {
        asmc_set_error("pcn: d=%d needs %zu B of LDS per wave (unsupported)", pd.d, per_wave);
        return ASMC_ERR_UNSUPPORTED;
    }
    const int64_t n_tiles = (n + 63) / 64;
    int blocks_per_cu = (int)((160 * 1024) / (lds_bytes + BM_TAB_N * 16));
    blocks_per_cu = blocks_per_cu < 1 ? 1 : (blocks_per_cu > 8 ? 8 : blocks_per_cu);
    int cap = ctx->num_cu * blocks_per_cu * 2;  // two rounds of resident blocks, grid-stride over tiles
    if (cap > ASMC_MAX_BLOCKS) cap = ASMC_MAX_BLOCKS;
    const int grid = grid_for(n_tiles, wpb, cap);
    *grid_out = grid;
    const int vec = pick_vec(rowbytes, x, x_prop ? (const void*)x_prop : (const void*)x);
    auto launch = [&](auto kern) {
        if (lds_bytes > 64 * 1024)
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        ASMC_LAUNCH(ctx, st, PHASE == 0 ? "k_pcn_step_generic" : "k_pcn_propose", kern, dim3(grid), dim3(wpb * 64), lds_bytes, st, n, x, ll, lp, lq, pd, rho_ptr, step,
                           block_counts, x_prop, qf_old, qf_new, wpb);
    };
    if (vec == 16)
        launch(k_pcn_step<T, 16, PHASE>);
    else if (vec == 8)
        launch(k_pcn_step<T, 8, PHASE>);
    else
        launch(k_pcn_step<T, 4, PHASE>);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

// ---- any d <= 128 on the fast kernels: zero-padding to the next supported width ------------------------------------------
// The register-resident kernels exist for d in {4, 8, 16, 32}, the matrix-core kernels for d in {64, 128}; every other d used
// to fall to the generic LDS kernel (6-9x slower).  A d-dimensional problem is the same as the D-dimensional one with
// x = (x, 0), mu = (mu, 0), L = diag(L, I), zero precisions on the padded coordinates of every density component, and NO
// noise on the padded coordinates (PcnDev.d_noise: y' = 0 there, |y|^2 and the Student-t dimension stay d's) - the real
// coordinates see exactly the arithmetic of the unpadded specification (same noise words: they are keyed by coordinate).
// Cost: two copy passes over the rows per call (pad, un-pad) and N x D x s bytes of scratch, grown on demand.
template <typename T>
__global__ __launch_bounds__(ASMC_BLOCK) void k_pad_rows(int64_t n, int d, int D, const T* __restrict__ x, T* __restrict__ xp) {
    const int64_t total = n * D, stride = (int64_t)gridDim.x * ASMC_BLOCK;
    for (int64_t e = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x; e < total; e += stride) {
        const int64_t i = e / D;
        const int j = (int)(e - i * D);
        xp[e] = j < d ? x[i * d + j] : (T)0;
    }
}
template <typename T>
__global__ __launch_bounds__(ASMC_BLOCK) void k_unpad_rows(int64_t n, int d, int D, const T* __restrict__ xp, T* __restrict__ x) {
    const int64_t total = n * d, stride = (int64_t)gridDim.x * ASMC_BLOCK;
    for (int64_t e = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x; e < total; e += stride) {
        const int64_t i = e / d;
        const int j = (int)(e - i * d);
        x[e] = xp[i * D + j];
    }
}
// padded tables: mu[D] | L[D, D] | Linv[D, D] | 3 x (mu[C_max, D] | prec[C_max, D]) for ll, lp, lq
__global__ __launch_bounds__(256) void k_pad_tables(int d, int D, PcnDev p, double* __restrict__ out) {
    double* mu = out;
    double* L = mu + D;
    double* Li = L + (size_t)D * D;
    for (int e = threadIdx.x; e < D; e += 256) mu[e] = e < d ? p.mu[e] : 0.0;
    for (int e = threadIdx.x; e < D * D; e += 256) {
        const int i = e / D, j = e - i * D;
        const bool in = i < d && j < d;
        L[e] = in ? p.L[i * d + j] : (i == j ? 1.0 : 0.0);
        Li[e] = in ? p.Linv[i * d + j] : (i == j ? 1.0 : 0.0);
    }
    const MixDev* mix[3] = {&p.ll, &p.lp, &p.lq};
    for (int k = 0; k < 3; k++) {
        double* m = Li + (size_t)D * D + (size_t)k * 2 * ASMC_MAX_COMPONENTS * D;
        double* pr = m + (size_t)ASMC_MAX_COMPONENTS * D;
        for (int e = threadIdx.x; e < mix[k]->C * D; e += 256) {
            const int c = e / D, j = e - c * D;
            m[e] = j < d ? mix[k]->mu[c * d + j] : 0.0;
            pr[e] = j < d ? mix[k]->prec[c * d + j] : 0.0;
        }
    }
}

int pcn_xpad_reserve(asmc_ctx* ctx, size_t need, hipStream_t st, const char* what) {
    if (need > ctx->xpad_bytes) {
        ASMC_HIP(hipStreamSynchronize(st));
        if (ctx->d_xpad) (void)hipFree(ctx->d_xpad);
        ctx->d_xpad = nullptr;
        ctx->xpad_bytes = 0;
        if (hipMalloc(&ctx->d_xpad, need) != hipSuccess) {
            (void)hipGetLastError();
            asmc_set_error("%s (%zu bytes)", what, need);
            return ASMC_ERR_NOMEM;
        }
        ctx->xpad_bytes = need;
    }
    return ASMC_OK;
}

int launch_pad_rows(asmc_ctx* ctx, int64_t n, int d, int D, int x_dtype, const void* src, void* dst, hipStream_t st) {
    const int grid = grid_for(n * D, ASMC_BLOCK * 4, ASMC_MAX_BLOCKS * 2);
    if (x_dtype == ASMC_F64)
        ASMC_LAUNCH(ctx, st, "k_pad_rows", k_pad_rows<double>, dim3(grid), dim3(ASMC_BLOCK), 0, st, n, d, D, (const double*)src, (double*)dst);
    else
        ASMC_LAUNCH(ctx, st, "k_pad_rows", k_pad_rows<float>, dim3(grid), dim3(ASMC_BLOCK), 0, st, n, d, D, (const float*)src, (float*)dst);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int launch_unpad_rows(asmc_ctx* ctx, int64_t n, int d, int D, int x_dtype, const void* src, void* dst, hipStream_t st) {
    const int grid = grid_for(n * D, ASMC_BLOCK * 4, ASMC_MAX_BLOCKS * 2);
    if (x_dtype == ASMC_F64)
        ASMC_LAUNCH(ctx, st, "k_unpad_rows", k_unpad_rows<double>, dim3(grid), dim3(ASMC_BLOCK), 0, st, n, d, D, (const double*)src, (double*)dst);
    else
        ASMC_LAUNCH(ctx, st, "k_unpad_rows", k_unpad_rows<float>, dim3(grid), dim3(ASMC_BLOCK), 0, st, n, d, D, (const float*)src, (float*)dst);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

// the padded problem in ctx->d_xpad (PcnPadded, asmc_pcn_shared.h)
int pcn_pad_problem(asmc_ctx* ctx, int64_t n, int d, int D, int x_dtype, const void* x, const PcnDev& src, int n_mix, hipStream_t st,
                    PcnPadded* out) {
    const size_t es = x_dtype == ASMC_F64 ? 8 : 4;
    const size_t tab_doubles = (size_t)D + 2 * (size_t)D * D + (n_mix ? 3 * 2 * (size_t)ASMC_MAX_COMPONENTS * D : 0);
    const size_t tab_bytes = ((tab_doubles * 8 + 255) / 256) * 256;
    const size_t row_bytes = (((size_t)n * D * es + 255) / 256) * 256;
    int rc = n_mix ? pcn_xpad_reserve(ctx, tab_bytes + (size_t)n * D * es, st, "pcn: no device memory for the zero-padded copy of the state")
                   : pcn_xpad_reserve(ctx, tab_bytes + 2 * row_bytes, st, "pcn: no device memory for the zero-padded copies of a proposal");
    if (rc) return rc;
    out->mu = reinterpret_cast<double*>(ctx->d_xpad);
    out->L = out->mu + D;
    out->Linv = out->L + (size_t)D * D;
    out->mix = out->Linv + (size_t)D * D;
    out->xp = reinterpret_cast<char*>(ctx->d_xpad) + tab_bytes;
    out->xq = n_mix ? nullptr : reinterpret_cast<char*>(out->xp) + row_bytes;
    ASMC_LAUNCH(ctx, st, "k_pad_tables", k_pad_tables, dim3(1), dim3(256), 0, st, d, D, src, out->mu);
    ASMC_LAUNCH_CHECK();
    return launch_pad_rows(ctx, n, d, D, x_dtype, x, out->xp, st);
}

// the same from a call's parameters: *p2 = *prm at dimension D, pointing at the padded tables; *xp: the padded rows
int pcn_pad_params(asmc_ctx* ctx, int64_t n, const void* x, const asmc_pcn_params* prm, int D, int n_mix, hipStream_t st,
                   asmc_pcn_params* p2, void** xp) {
    PcnDev src;
    memset(&src, 0, sizeof(src));
    src.mu = prm->mu_dev, src.L = prm->L_dev, src.Linv = prm->Linv_dev;
    src.ll = to_dev(prm->log_likelihood), src.lp = to_dev(prm->log_prior);
    src.lq = n_mix == 3 ? to_dev(prm->log_q) : src.lp;  // (two: a placeholder - the proposal density is the flow)
    PcnPadded pad;
    const int rc = pcn_pad_problem(ctx, n, prm->d, D, prm->x_dtype, x, src, n_mix, st, &pad);
    if (rc) return rc;
    *p2 = *prm;
    p2->d = D;
    p2->mu_dev = pad.mu;
    p2->L_dev = pad.L;
    p2->Linv_dev = pad.Linv;
    asmc_mixture* mix[3] = {&p2->log_likelihood, &p2->log_prior, &p2->log_q};
    for (int k = 0; k < n_mix; k++) {
        mix[k]->mu_dev = pad.mix + (size_t)k * 2 * ASMC_MAX_COMPONENTS * D;
        mix[k]->prec_dev = mix[k]->mu_dev + (size_t)ASMC_MAX_COMPONENTS * D;
    }
    *xp = pad.xp;
    return ASMC_OK;
}

// coordinate-major scratch for the whitened state of one mutation (grown on demand, kept for the life of the ctx);
// false when the device has no room for it (callers then stay on the in-place row-major path)
bool pcn_ensure_ysoa(asmc_ctx* ctx, int64_t n, int d, int x_dtype, PcnDev& pd, hipStream_t st, bool with_scratch) {
    if (pcn_env_aos()) return false;
    const int64_t n_pad = ((n + 63) / 64) * 64;
    const size_t one = (size_t)n_pad * d * (x_dtype == ASMC_F64 ? 8 : 4);
    if (one >= (1ULL << 32)) return false;  // the kernels address the buffer through one 32-bit-offset descriptor
    const size_t need = with_scratch ? 2 * one : one;  // fused flow step: y' scratch of the same layout behind the state
    if (need > ctx->ysoa_bytes) {
        if (hipStreamSynchronize(st) != hipSuccess) return false;
        if (ctx->d_ysoa) (void)hipFree(ctx->d_ysoa);
        ctx->d_ysoa = nullptr;
        ctx->ysoa_bytes = 0;
        if (hipMalloc(&ctx->d_ysoa, need) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        ctx->ysoa_bytes = need;
        // the fused flow step reads whole 64-particle tiles: the slots behind a ragged last tile must hold finite numbers
        if (hipMemsetAsync(ctx->d_ysoa, 0, need, st) != hipSuccess) return false;
    }
    pd.ys = ctx->d_ysoa;
    pd.n_pad = n_pad;
    return true;
}

// The reference checks the carried log q for NaN after every mutation (smc/minipcn.py: "Log proposal contains NaN values").
// The count rides on the mutation call's own read-back instead of a call and a synchronisation of its own: NaN / inf counts
// of lq -> HP_PCN_LQ_COUNTS, read by asmc_pcn_lq_nan after the call's synchronisation.
int pcn_enqueue_lq_check(asmc_ctx* ctx, int64_t n, const double* lq, hipStream_t st) {
    const int rc = asmc_count_nonfinite_enqueue(ctx, n, lq, st);
    if (rc) return rc;
    ASMC_HIP(hipMemcpyAsync(ctx->h_pinned + HP_PCN_LQ_COUNTS, asmc_count_slot(ctx), sizeof(unsigned long long) * 2, hipMemcpyDeviceToHost, st));
    return ASMC_OK;
}

// A mutation call's read-back into the pinned HP_PCN_* cells (asmc_scratch.h): accept counts | step sizes | rho.
// d_bad == NULL: counts, history and rho (-> HP_PCN_RHO) in a copy each.  Flow steps pass their non-finite-density counter: d_rho's
// head and the history then come in ONE copy (d_rho_hist = d_rho + 8: rho lands in HP_PCN_RHO_HEAD) and *d_bad -> HP_PCN_NONFINITE.
int pcn_readback_enqueue(asmc_ctx* ctx, int n_steps, const void* d_bad, hipStream_t st) {
    double* h = ctx->h_pinned;
    ASMC_HIP(hipMemcpyAsync(h + HP_PCN_COUNTS, ctx->d_counts, sizeof(long long) * n_steps, hipMemcpyDeviceToHost, st));
    if (!d_bad) {
        ASMC_HIP(hipMemcpyAsync(h + HP_PCN_RHO_HIST, ctx->d_rho + 8, sizeof(double) * n_steps, hipMemcpyDeviceToHost, st));
        ASMC_HIP(hipMemcpyAsync(h + HP_PCN_RHO, ctx->d_rho, sizeof(double), hipMemcpyDeviceToHost, st));
    } else {
        ASMC_HIP(hipMemcpyAsync(h + HP_PCN_RHO_HEAD, ctx->d_rho, sizeof(double) * (8 + n_steps), hipMemcpyDeviceToHost, st));
        ASMC_HIP(hipMemcpyAsync(h + HP_PCN_NONFINITE, d_bad, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    }
    return ASMC_OK;
}
// ... handed out once the caller has waited for it.  flow: pcn_readback_enqueue had a d_bad; lq_checked: pcn_enqueue_lq_check
// followed it
void pcn_readback_handout(asmc_ctx* ctx, int n_steps, bool flow, bool lq_checked, double* rho_out_host, int64_t* n_accept_host,
                          double* rho_hist_host) {
    const long long* h_counts = reinterpret_cast<const long long*>(ctx->h_pinned + HP_PCN_COUNTS);
    const double* h_rho_hist = ctx->h_pinned + HP_PCN_RHO_HIST;
    if (lq_checked) memcpy(&ctx->lq_nan, ctx->h_pinned + HP_PCN_LQ_COUNTS, sizeof(unsigned long long));
    for (int t = 0; t < n_steps; t++) n_accept_host[t] = (int64_t)h_counts[t];
    if (rho_hist_host)
        for (int t = 0; t < n_steps; t++) rho_hist_host[t] = h_rho_hist[t];
    *rho_out_host = ctx->h_pinned[flow ? HP_PCN_RHO_HEAD : HP_PCN_RHO];
    if (flow) memcpy(&ctx->flow_nonfinite, ctx->h_pinned + HP_PCN_NONFINITE, sizeof(unsigned long long));  // fused steps only (else stale zero)
}

// packs the transform epilogue's table (TRTAB_*) from the device-resident transform / premap / mixture tables
extern "C" __global__ void k_trtab_pack(int d, const int* __restrict__ kind, const double* __restrict__ lower, const double* __restrict__ upper,
                             const double* __restrict__ mean, const double* __restrict__ sd, const double* __restrict__ premap,
                             const double* __restrict__ q_logw, const double* __restrict__ q_mu, const double* __restrict__ q_prec,
                             double eps, double unit_logj, double affine_logj, int minus_logj, double* __restrict__ out) {
    const int j = threadIdx.x;
    if (j < d) {
        out[j] = (double)kind[j];
        out[d + j] = lower[j];
        out[2 * d + j] = upper[j];
        out[3 * d + j] = mean ? mean[j] : 0.0;
        out[4 * d + j] = sd ? sd[j] : 1.0;
        out[5 * d + j] = 1.0 / (upper[j] - lower[j]);
        out[6 * d + j] = sd ? 1.0 / sd[j] : 1.0;
        for (int r = 0; r < 5; r++) out[(7 + r) * d + j] = premap ? premap[r * d + j] : 0.0;
        out[12 * d + j] = q_mu ? q_mu[j] : 0.0;
        out[13 * d + j] = q_prec ? q_prec[j] : 0.0;
    }
    if (j == 0) {
        double* sc = out + TRTAB_ROWS * d;
        sc[0] = eps, sc[1] = unit_logj, sc[2] = affine_logj, sc[3] = mean ? 1.0 : 0.0;
        sc[4] = q_logw ? q_logw[0] : 0.0, sc[5] = premap ? 1.0 : 0.0, sc[6] = minus_logj ? 1.0 : 0.0, sc[7] = 0.0;
    }
}

// =============================================================================================
// the launch interface of asmc_pcn_drive.hip (asmc_pcn_shared.h): the call's x_dtype becomes the template argument here
// =============================================================================================
int pcn_step_launch(asmc_ctx* ctx, int64_t n, int x_dtype, void* x, double* ll, double* lp, double* lq, const PcnDev& pd,
                    const double* rho_ptr, uint32_t step, long long* block_counts, int* grid_out, hipStream_t st) {
    if (x_dtype == ASMC_F64)
        return launch_pcn_step<double, 0>(ctx, n, (double*)x, ll, lp, lq, pd, rho_ptr, step, block_counts, grid_out, nullptr, nullptr, nullptr, st);
    return launch_pcn_step<float, 0>(ctx, n, (float*)x, ll, lp, lq, pd, rho_ptr, step, block_counts, grid_out, nullptr, nullptr, nullptr, st);
}

int pcn_generic_propose_launch(asmc_ctx* ctx, int64_t n, int x_dtype, const void* x, void* x_prop, double* qf_old, double* qf_new,
                               const PcnDev& pd, const double* rho_ptr, uint32_t step, int* grid_out, hipStream_t st) {
    if (x_dtype == ASMC_F64)
        return launch_pcn_step<double, 1>(ctx, n, (double*)const_cast<void*>(x), nullptr, nullptr, nullptr, pd, rho_ptr, step, nullptr,
                                          grid_out, (double*)x_prop, qf_old, qf_new, st);
    return launch_pcn_step<float, 1>(ctx, n, (float*)const_cast<void*>(x), nullptr, nullptr, nullptr, pd, rho_ptr, step, nullptr, grid_out,
                                     (float*)x_prop, qf_old, qf_new, st);
}

template <typename T>
static int pcn_reg_flow_launch_t(asmc_ctx* ctx, int64_t n, int mode, T* y, T* x_prop, double* ll, double* lp, double* lq, double* ll_new,
                                 double* lp_new, const double* lq_new, const PcnDev& pd, const double* rho_ptr, uint32_t step,
                                 long long* block_counts, int* grid_out, hipStream_t st) {
    switch (mode) {
#define PCN_FLOW_MODE(MD) \
    case MD:              \
        return dispatch_pcn_reg_flow<T, MD>(ctx, n, y, x_prop, ll, lp, lq, ll_new, lp_new, lq_new, pd, rho_ptr, step, block_counts, grid_out, st);
        PCN_FLOW_MODE(PCN_FLOW_PROPOSE)
        PCN_FLOW_MODE(PCN_FLOW_ACCEPT)
        PCN_FLOW_MODE(PCN_FLOW_PROPOSE_S)
        PCN_FLOW_MODE(PCN_FLOW_ACCEPT_S)
        PCN_FLOW_MODE(PCN_FLOW_PROPOSE_SX)
        PCN_FLOW_MODE(PCN_FLOW_ACCEPT_SJ)
        PCN_FLOW_MODE(PCN_FLOW_PROPOSE_SXT_LOGIT)
        PCN_FLOW_MODE(PCN_FLOW_PROPOSE_SXT_PROBIT)
#undef PCN_FLOW_MODE
        default: break;
    }
    asmc_set_error("pcn flow: no kernel for mode %d", mode);
    return ASMC_ERR_UNSUPPORTED;
}

int pcn_reg_flow_launch(asmc_ctx* ctx, int64_t n, int x_dtype, int mode, void* y, void* x_prop, double* ll, double* lp, double* lq,
                        double* ll_new, double* lp_new, const double* lq_new, const PcnDev& pd, const double* rho_ptr, uint32_t step,
                        long long* block_counts, int* grid_out, hipStream_t st) {
    if (x_dtype == ASMC_F64)
        return pcn_reg_flow_launch_t<double>(ctx, n, mode, (double*)y, (double*)x_prop, ll, lp, lq, ll_new, lp_new, lq_new, pd, rho_ptr, step,
                                             block_counts, grid_out, st);
    // PCN_FLOW_ACCEPT_SJ: y / x_prop carry the fp64 log-Jacobian arrays whatever the storage type - the kernel's parameters are
    // T* (coordinate-major accept reads no state through them) and it reads the two as doubles again
    return pcn_reg_flow_launch_t<float>(ctx, n, mode, static_cast<float*>(y), static_cast<float*>(x_prop), ll, lp, lq, ll_new, lp_new, lq_new,
                                        pd, rho_ptr, step, block_counts, grid_out, st);
}

int pcn_set_scalar_launch(asmc_ctx* ctx, double* cell, double v, hipStream_t st) {
    ASMC_LAUNCH(ctx, st, "k_set_scalar", k_set_scalar, dim3(1), dim3(1), 0, st, cell, v);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int pcn_accept_flags_launch(asmc_ctx* ctx, int64_t n, double* ll, double* lp, double* lq, const double* ll_new, const double* lp_new,
                            const double* lq_new, double* lj_old, const double* lj_new, const double* qf_old, const double* qf_new,
                            double beta, uint64_t seed, uint64_t gid0, uint32_t step, hipStream_t st) {
    ASMC_HIP(hipMemsetAsync(ctx->d_keys, 0, sizeof(unsigned long long), st));
    const int grid = grid_for(n, ASMC_BLOCK * 2, ASMC_MAX_BLOCKS);
    ASMC_LAUNCH(ctx, st, "k_pcn_accept_flags", k_pcn_accept_flags, dim3(grid), dim3(ASMC_BLOCK), 0, st, n, ll, lp, lq, ll_new, lp_new, lq_new,
                lj_old, lj_new, qf_old, qf_new, beta, (unsigned long long)seed, (unsigned long long)gid0, step, ctx->d_flags, ctx->d_keys);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int pcn_adapt_exchanged_launch(asmc_ctx* ctx, int t, double target, int adapt, int lag, hipStream_t st) {
    double* d_rho_hist = ctx->d_rho + 8;
    ASMC_LAUNCH(ctx, st, "k_pcn_adapt", k_pcn_adapt, dim3(1), dim3(1024), 0, st, 1, (const long long*)ctx->count_cell, ctx->count_n_global, t,
                ctx->d_counts, ctx->d_rho, d_rho_hist, target, adapt, (const double*)(d_rho_hist + t), 1,
                lag > 1 ? (const long long*)ctx->count_cell : (const long long*)nullptr);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int pcn_trtab_pack_launch(asmc_ctx* ctx, int d, const asmc_transform* t, const double* premap_dev, const asmc_mixture* qmix,
                          int minus_logj, double* d_tab, hipStream_t st) {
    ASMC_LAUNCH(ctx, st, "k_trtab_pack", k_trtab_pack, dim3(1), dim3(64), 0, st, d, t->kind_dev, t->lower_dev, t->upper_dev,
                t->mean_dev, t->std_dev, premap_dev, qmix ? qmix->logw_dev : (const double*)nullptr,
                qmix ? qmix->mu_dev : (const double*)nullptr, qmix ? qmix->prec_dev : (const double*)nullptr, t->eps, t->unit_logj,
                t->affine_logj, minus_logj, d_tab);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}
