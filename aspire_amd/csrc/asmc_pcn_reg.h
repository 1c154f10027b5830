// asmc_pcn_reg.h - the register-resident pCN step body (d == D at compile time) and the gather of its packed parameter block,
// shared by the kernels that instantiate it: k_pcn_reg (asmc_pcn.hip) and the rung-batched k_pt_reg (asmc_pt_steps.hip).
#pragma once
#include "asmc_pcn_shared.h"

// =============================================================================================
// fused pCN step, register resident (d == D, compile time): one particle per lane, the working
// vector v[D] lives in VGPRs, L / Linv / mu / target parameters are wave-uniform scalar loads, both
// triangular mat-vecs are fully unrolled FMA chains.  Rows travel HBM <-> LDS tile <-> registers
// with 16-B accesses on every hop.
// =============================================================================================
template <typename T, int D>
__device__ __forceinline__ void row_to_regs(const char* row, double (&v)[D]) {
    constexpr int ROWB = D * (int)sizeof(T);
#pragma unroll
    for (int c = 0; c < ROWB / 16; c++) {
        const uint4 q = *reinterpret_cast<const uint4*>(row + 16 * c);
        if (sizeof(T) == 8) {
            v[2 * c] = __longlong_as_double(((long long)q.y << 32) | (long long)q.x);
            v[2 * c + 1] = __longlong_as_double(((long long)q.w << 32) | (long long)q.z);
        } else {
            v[4 * c] = (double)__uint_as_float(q.x);
            v[4 * c + 1] = (double)__uint_as_float(q.y);
            v[4 * c + 2] = (double)__uint_as_float(q.z);
            v[4 * c + 3] = (double)__uint_as_float(q.w);
        }
    }
}

template <typename T, int D>
__device__ __forceinline__ void regs_to_row(char* row, const double (&v)[D]) {
    constexpr int ROWB = D * (int)sizeof(T);
#pragma unroll
    for (int c = 0; c < ROWB / 16; c++) {
        uint4 q;
        if (sizeof(T) == 8) {
            const long long a = __double_as_longlong(v[2 * c]), b = __double_as_longlong(v[2 * c + 1]);
            q.x = (uint32_t)a;
            q.y = (uint32_t)(a >> 32);
            q.z = (uint32_t)b;
            q.w = (uint32_t)(b >> 32);
        } else {
            q.x = __float_as_uint((float)v[4 * c]);
            q.y = __float_as_uint((float)v[4 * c + 1]);
            q.z = __float_as_uint((float)v[4 * c + 2]);
            q.w = __float_as_uint((float)v[4 * c + 3]);
        }
        *reinterpret_cast<uint4*>(row + 16 * c) = q;
    }
}

template <int D>
__device__ __forceinline__ double mixture_eval_regs(const MixDev& m, const double (&v)[D]) {
    // component 0 (the only one for plain Gaussians): no exp/log
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < D; j++) {
        const double t = v[j] - m.mu[j];
        q = fma(t * t, m.prec[j], q);
    }
    double best = m.logw[0] - 0.5 * q;
    if (m.C == 1) return best;
    // further components: running (max, sum) log-sum-exp; runtime loop keeps the code small
    double s = 1.0;
#pragma unroll 1
    for (int c = 1; c < m.C; c++) {
        const double* __restrict__ mu = m.mu + c * D;
        const double* __restrict__ pr = m.prec + c * D;
        double qc = 0.0;
#pragma unroll
        for (int j = 0; j < D; j++) {
            const double t = v[j] - mu[j];
            qc = fma(t * t, pr[j], qc);
        }
        const double tc = m.logw[c] - 0.5 * qc;
        if (tc > best) {
            s = fma(s, exp(best - tc), 1.0);
            best = tc;
        } else if (tc > -INFINITY) {
            s += exp(tc - best);
        }
    }
    // (a row with a NaN coordinate: the first term is NaN, no comparison above holds and best + log(s) is NaN - DESIGN.md §3.15)
    return best == -INFINITY ? -INFINITY : best + log(s);
}

// All read-only tables are packed into ONE `const __restrict__` buffer (ctx scratch, filled per mutate call):
// only a noalias kernel argument lets LLVM prove the tables are not clobbered by the particle stores and
// select scalar (s_load) instead of vector loads, and one base pointer keeps the SGPR budget for data.
// L and Linv are stored as PACKED lower triangles (row j at j(j+1)/2): 2 x 4.2 KB at d = 32, so that everything a
// step touches (~10 KB) stays inside the 16 KB scalar data cache (dense 2 x 8 KB tables thrashed it).
// layout (doubles): Ltri[D(D+1)/2] | Linvtri[D(D+1)/2] | mu[D] | 3 x { logw[8] | mu[8*D] | prec[8*D] }  (ll, lp, lq)
// v <- A v for a lower-triangular A stored packed by rows (wave-uniform, read through scalar loads), in place.
// Descending row groups of RG: rows j0-RG+1..j0 only read v[0..j0], which later (lower) groups never need
// overwritten entries of, so the update is legal in place.
template <int D>
__device__ __forceinline__ void tri_matvec_inplace(const double* __restrict__ A, double (&v)[D]) {
    constexpr int RG = D >= 4 ? 4 : D;
#pragma unroll
    for (int g = D / RG - 1; g >= 0; g--) {
        const int j0 = g * RG;  // rows j0 .. j0+RG-1
        double s[RG];
#pragma unroll
        for (int r = 0; r < RG; r++) s[r] = 0.0;
#pragma unroll
        for (int k = 0; k < j0 + RG; k++) {
#pragma unroll
            for (int r = 0; r < RG; r++)
                if (k <= j0 + r) s[r] = fma(A[(j0 + r) * (j0 + r + 1) / 2 + k], v[k], s[r]);
        }
#pragma unroll
        for (int r = 0; r < RG; r++) v[j0 + r] = s[r];
    }
}

// (the modes of k_pcn_reg - PCN_X_STEP .. PCN_Y_STEP_TSG - are listed and described in asmc_pcn_shared.h: the drivers name them)

// 64-row tile copies for rows of `dr` < D elements (PCN_X_PROPOSE_PAD): fully unrolled, element-wise coalesced
// accesses, row index by multiplication with magic = floor(2^32 / dr) + 1 (exact for e < 2^16) - no run-time loop, no
// division (a loop here brings back the scalar-load hoisting described above)
template <typename T, int D>
__device__ __forceinline__ void pad_tile_load(const T* __restrict__ g, int64_t valid_elems, int dr, unsigned magic, int ldsrow,
                                              char* lds, int lane) {
#pragma unroll
    for (int it = 0; it < D; it++) {
        const int e = it * 64 + lane;
        if (e < 64 * dr) {
            const int r = (int)__umulhi((unsigned)e, magic), c = e - r * dr;
            T v = (T)0;
            if (e < valid_elems) v = g[e];
            reinterpret_cast<T*>(lds + r * ldsrow)[c] = v;
        }
    }
}
template <typename T, int D>
__device__ __forceinline__ void pad_tile_store_rows(T* __restrict__ g, int64_t valid_elems, int dr, unsigned magic, int ldsrow,
                                                    const char* lds, int lane, unsigned long long rowmask) {
#pragma unroll
    for (int it = 0; it < D; it++) {
        const int e = it * 64 + lane;
        if (e < 64 * dr && e < valid_elems) {
            const int r = (int)__umulhi((unsigned)e, magic), c = e - r * dr;
            if ((rowmask >> r) & 1ULL) g[e] = reinterpret_cast<const T*>(lds + r * ldsrow)[c];
        }
    }
}

template <typename T, int D, int NOISE, int MODE>
__device__ __forceinline__ void pcn_reg_body(int64_t n, T* __restrict__ x, double* __restrict__ ll,
                                             double* __restrict__ lp, double* __restrict__ lq,
                                             const double* __restrict__ ptab, const PcnScalars& p,
                                             const double* __restrict__ rho_ptr, uint32_t step,
                                             long long* __restrict__ block_counts) {
    extern __shared__ __align__(16) char smem[];
    constexpr bool TP = MODE == PCN_X_STEP_T || MODE == PCN_Y_STEP_T || MODE == PCN_Y_STEP_TS || MODE == PCN_X_PROPOSE_T ||
                        MODE == PCN_X_PROPOSE_PAD_T || MODE == PCN_Y_STEP_TSG;
    constexpr bool GEN = MODE == PCN_Y_STEP_SG || MODE == PCN_Y_STEP_TSG;  // general mixtures on the whitened state
    constexpr bool SOA = (MODE >= PCN_WHITEN_S && MODE <= PCN_UNWHITEN_XS) || GEN;
    constexpr bool PAD = MODE == PCN_X_PROPOSE_PAD || MODE == PCN_X_PROPOSE_PAD_T;
    constexpr bool PROPOSE = MODE == PCN_X_PROPOSE || MODE == PCN_X_PROPOSE_T || PAD;
    constexpr int M = PROPOSE ? PCN_X_STEP : GEN ? PCN_Y_STEP : MODE == PCN_WHITEN_S ? PCN_WHITEN : (MODE == PCN_Y_STEP_S || MODE == PCN_Y_STEP_TS) ? PCN_Y_STEP
                      : MODE == PCN_UNWHITEN_S ? PCN_UNWHITEN : MODE == PCN_UNWHITEN_XS ? PCN_UNWHITEN_X
                      : TP ? MODE - PCN_X_STEP_T : MODE;
    constexpr bool ROW_IN = !SOA || M == PCN_WHITEN;     // the state arrives as row-major x through the LDS tile
    constexpr bool ROW_OUT = !SOA || M == PCN_UNWHITEN || M == PCN_UNWHITEN_X;  // ... leaves that way
    T* __restrict__ ys = reinterpret_cast<T*>(p.ys);
    constexpr int ROWB = D * (int)sizeof(T);
    constexpr int LDSROW = ROWB + 16;
    const int WPB = (int)(blockDim.x >> 6);  // waves per block: chosen by the launcher from the LDS budget
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int dr = PAD ? p.d_real : D;                                       // elements per stored row
    const int dn = (p.d_noise > 0 && p.d_noise < D) ? p.d_noise : D;         // real dimension of a zero-padded problem (asmc_pcn_mutate)
    const int rowb = PAD ? dr * (int)sizeof(T) : ROWB;
    const int ldsrow = PAD ? lds_row_stride(rowb) : LDSROW;
    char* tile = smem + (size_t)wave * 64 * LDSROW;
    char* myrow = tile + lane * ldsrow;
    const double rho = *rho_ptr;
    const double a = sqrt(1.0 - rho * rho);
    long long n_acc = 0;
    const int64_t n_tiles = (n + 63) / 64;
    // the Box-Muller tables of the default noise, staged by the whole block (the only block-wide barrier of the kernel)
    bm_d2* bmt = nullptr;
    if constexpr (NOISE == ASMC_NOISE_F64 && (M == PCN_X_STEP || M == PCN_Y_STEP)) {
        bmt = bm_lds();
        bm_tab_stage_rt(bmt, p.bmtab);
        __syncthreads();
    }
    // one 64-particle tile per wave and NO tile loop: with a loop LLVM hoists the ~1300 loop-invariant
    // table loads and the fp64 polynomial constants out of it and then spills them
    const int64_t t = (int64_t)blockIdx.x * WPB + wave;
    if (t < n_tiles) {
        const bool active = true;
        const int64_t row0 = t * 64;
        const int64_t i = row0 + lane;
        // coordinate-major state: wave-uniform tile base (scalar registers) + the lane as a 32-bit offset
        // descriptor over the whole scratch buffer, built from wave-uniform values only (< 4 GB: checked by the host)
        const unsigned long long ysa = (unsigned long long)(uintptr_t)ys;
        T* ysu = reinterpret_cast<T*>(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(ysa >> 32)) << 32) |
                                      (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)ysa));
        // after fused flow steps a tile's state lives in the half of the allocation its parity byte names (asmc_pcn_fused.hip)
        if (M == PCN_UNWHITEN_X && SOA && p.tile_par != nullptr && __builtin_amdgcn_readfirstlane((int)p.tile_par[t]) != 0)
            ysu += (size_t)__builtin_amdgcn_readfirstlane((int)(unsigned)p.n_pad) * D;
        const __amdgpu_buffer_rsrc_t ysr = __builtin_amdgcn_make_buffer_rsrc(
            ysu, 0, SOA ? (int)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)p.n_pad * D * sizeof(T))) : 0,
            0x00020000);
        const unsigned ys_tile = (unsigned)__builtin_amdgcn_readfirstlane((int)t) * 64u * (unsigned)sizeof(T);
        const unsigned ys_row = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)p.n_pad) * (unsigned)sizeof(T);
        const unsigned ys_lane = (unsigned)lane * (unsigned)sizeof(T);
        const bool valid = active && i < n;
        const int64_t valid_bytes = active ? (((n - row0) < 64 ? (n - row0) : 64) * (int64_t)rowb) : 0;
        char* gbase = reinterpret_cast<char*>(x) + row0 * rowb;
        const unsigned magic = PAD ? 0xFFFFFFFFu / (unsigned)dr + 1u : 0u;
        if (PAD)
            pad_tile_load<T, D>(reinterpret_cast<const T*>(gbase), valid_bytes / (int64_t)sizeof(T), dr, magic, ldsrow, tile, lane);
        else if (active && ROW_IN)
            tile_load<16>(gbase, valid_bytes, ROWB, LDSROW, tile, lane);
        double oll = 0.0, olp = 0.0, olq = 0.0;
        if (valid && !PROPOSE && (M == PCN_X_STEP || M == PCN_Y_STEP)) {
            oll = ll[i];
            olp = lp[i];
            olq = lq[i];
        }
        wave_lds_sync();
        bool acc = false;
        const long zoff = 0;
        const double* __restrict__ tab = ptab + zoff;
        const double* __restrict__ Lp = tab;
        const double* __restrict__ Lip = tab + PTAB_TRI(D);
        const double* __restrict__ mup = tab + 2 * PTAB_TRI(D);
        const double* __restrict__ m0 = tab + 2 * PTAB_TRI(D) + D;
        const MixDev mll = {p.c_ll, m0, m0 + ASMC_MAX_COMPONENTS, m0 + ASMC_MAX_COMPONENTS * (1 + D)};
        const MixDev mlp = {p.c_lp, m0 + PTAB_MIX(D), m0 + PTAB_MIX(D) + ASMC_MAX_COMPONENTS,
                            m0 + PTAB_MIX(D) + ASMC_MAX_COMPONENTS * (1 + D)};
        const MixDev mlq = {p.c_lq, m0 + 2 * PTAB_MIX(D), m0 + 2 * PTAB_MIX(D) + ASMC_MAX_COMPONENTS,
                            m0 + 2 * PTAB_MIX(D) + ASMC_MAX_COMPONENTS * (1 + D)};
        if (valid) {
            const unsigned long long gid = p.gid0 + (unsigned long long)i;
            double v[D];
            if (PAD) {
#pragma unroll
                for (int j = 0; j < D; j++) v[j] = j < dr ? row_get<T>(myrow, j) : 0.0;  // padded mu is zero too
            } else if (ROW_IN) {
                row_to_regs<T, D>(myrow, v);
            } else {
#pragma unroll
                for (int j = 0; j < D; j++) v[j] = soa_load<T>(ysr, ys_lane, ys_tile + (unsigned)j * ys_row);
            }
            if (M == PCN_WHITEN) {
#pragma unroll
                for (int j = 0; j < D; j++) v[j] -= mup[j];
                tri_matvec_inplace<D>(Lip, v);
                if (SOA) {
#pragma unroll
                    for (int j = 0; j < D; j++) soa_store<T>(ysr, ys_lane, ys_tile + (unsigned)j * ys_row, v[j]);
                } else {
#pragma unroll
                    for (int j = 0; j < D; j++) v[j] = (double)(T)v[j];
                    regs_to_row<T, D>(myrow, v);
                    acc = true;
                }
            } else if (M == PCN_UNWHITEN || M == PCN_UNWHITEN_X) {
                tri_matvec_inplace<D>(Lp, v);
#pragma unroll
                for (int j = 0; j < D; j++) v[j] = (double)(T)(mup[j] + v[j]);
                if (M == PCN_UNWHITEN) {
                    ll[i] = mixture_eval_regs<D>(mll, v);
                    lp[i] = mixture_eval_regs<D>(mlp, v);
                    lq[i] = mixture_eval_regs<D>(mlq, v);
                }
                regs_to_row<T, D>(myrow, v);
                acc = true;
            } else {
                double q0 = 0.0;
                if (M == PCN_X_STEP) {
#pragma unroll
                    for (int j = 0; j < D; j++) v[j] -= mup[j];
                    // y = Linv (x - mu), in place, 4 interleaved FMA chains per row group
#ifndef ASMC_ABLATE_MATVEC
                    tri_matvec_inplace<D>(Lip, v);
#endif
                }
#pragma unroll
                for (int j = 0; j < D; j++) q0 = fma(v[j], v[j], q0);
                // y' = a y + rho sqrt(s) xi (rounded to the storage type when y is what gets stored); q1 = |y'|^2
                double q1 = 0.0;
                const double rs = tpcn_scale_ct<TP>(rho, p.nu, q0, p.gam, i);
                if (NOISE == ASMC_NOISE_F64) {
#pragma unroll
                    for (int qd = 0; qd < (D + 3) / 4; qd++) {
                        double z[4];
                        normal_quad(p.seed, gid, step, (uint32_t)qd, bmt, z[0], z[1], z[2], z[3]);
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            if (4 * qd + e < D) {
                                v[4 * qd + e] = fma(rs, z[e], a * v[4 * qd + e]);
                                if (M == PCN_Y_STEP) v[4 * qd + e] = (double)(T)v[4 * qd + e];
                                q1 = fma(v[4 * qd + e], v[4 * qd + e], q1);
                            }
                        }
                        __builtin_amdgcn_sched_barrier(0);  // one block at a time (register pressure)
                    }
                } else {
#pragma unroll
                    for (int qd = 0; qd < D / 4; qd++) {
                        double z[4];
#ifndef ASMC_ABLATE_NOISE
                        normal_quad_f32(p.seed, gid, step, (uint32_t)qd, z[0], z[1], z[2], z[3]);
#else
                        z[0] = z[1] = z[2] = z[3] = 0.25 * (double)(lane + qd);
#endif
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            v[4 * qd + e] = fma(rs, z[e], a * v[4 * qd + e]);
                            if (M == PCN_Y_STEP) v[4 * qd + e] = (double)(T)v[4 * qd + e];
                            q1 = fma(v[4 * qd + e], v[4 * qd + e], q1);
                        }
                        if (qd & 1) __builtin_amdgcn_sched_barrier(0);
                    }
                }
                if (PAD || dn < D) {  // the padded coordinates carry no noise: y' = 0 there, and they stay out of |y'|^2
                    const int dm = PAD ? dr : dn;  // (dn < D: a wave-uniform branch that only zero-padded problems take)
                    q1 = 0.0;
#pragma unroll
                    for (int j = 0; j < D; j++) {
                        v[j] = j < dm ? v[j] : 0.0;
                        q1 = fma(v[j], v[j], q1);
                    }
                }
                double nll, nlp, nlq;
                if (M == PCN_X_STEP) {
                    // x' = mu + L y', rounded to the storage type
#ifndef ASMC_ABLATE_MATVEC
                    tri_matvec_inplace<D>(Lp, v);
#endif
#pragma unroll
                    for (int j = 0; j < D; j++) v[j] = (double)(T)(mup[j] + v[j]);
                    if (PROPOSE) {
                        ll[i] = 2.0 * ref_corr_ct<TP>(q0, p.nu, PAD ? dr : dn);
                        lp[i] = 2.0 * ref_corr_ct<TP>(q1, p.nu, PAD ? dr : dn);
                        if (PAD) {
#pragma unroll
                            for (int j = 0; j < D; j++)
                                if (j < dr) row_set<T>(myrow, j, v[j]);
                        } else {
                            regs_to_row<T, D>(myrow, v);
                        }
                        acc = true;
                    }
#ifndef ASMC_ABLATE_TARGET
                    if (!PROPOSE) {
                        nll = mixture_eval_regs<D>(mll, v);
                        nlp = mixture_eval_regs<D>(mlp, v);
                        nlq = mixture_eval_regs<D>(mlq, v);
                    } else {
                        nll = nlp = nlq = 0.0;
                    }
#else
                    nll = v[0], nlp = v[1], nlq = v[2];
#endif
                } else if (GEN) {
                    // v keeps y'; x' goes to a second register array for the general mixture evaluation
                    double xq[D];
#pragma unroll
                    for (int g = 0; g < D / 4; g++) {
                        const int j0 = 4 * g;
                        double sr[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                        for (int k = 0; k < j0 + 4; k++) {
#pragma unroll
                            for (int r = 0; r < 4; r++)
                                if (k <= j0 + r) sr[r] = fma(Lp[(j0 + r) * (j0 + r + 1) / 2 + k], v[k], sr[r]);
                        }
#pragma unroll
                        for (int r = 0; r < 4; r++) xq[j0 + r] = (double)(T)(mup[j0 + r] + sr[r]);
                    }
                    nll = mixture_eval_regs<D>(mll, xq);
                    nlp = mixture_eval_regs<D>(mlp, xq);
                    nlq = mixture_eval_regs<D>(mlq, xq);
                } else {
                    // v keeps y' (it is what gets stored); x'_j = mu_j + sum_k L[j,k] y'_k is produced four rows
                    // at a time and folded straight into the three quadratic forms (component 0 of each target)
                    double qa = 0.0, qb = 0.0, qc = 0.0;
                    // L comes from the BLOCKED copy of the table (PTAB_BLK): sixteen consecutive doubles per 4 x 4 block, in the order of
                    // use.  Read from the row-packed triangle the scalar loads were merged into 64-byte pieces that straddle row groups -
                    // data loaded long before its use, which the pCN instantiation then parked in vector-register lanes: 1 134
                    // v_writelane / v_readlane per tile next to 1 092 fp64 FMAs (round 5's generated code).  Same products, same order.
                    const double* __restrict__ Lb = tab + PTAB_SIZE(D);
#pragma unroll
                    for (int g = 0; g < D / 4; g++) {
                        const int j0 = 4 * g;
                        double sr[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                        for (int k = 0; k < j0 + 4; k++) {
#pragma unroll
                            for (int r = 0; r < 4; r++)
                                if (k <= j0 + r) sr[r] = fma(Lb[16 * (g * (g + 1) / 2 + k / 4) + 4 * (k % 4) + r], v[k], sr[r]);
                        }
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            const int j = j0 + r;
                            const double xj = (double)(T)(mup[j] + sr[r]);
                            const double ta = xj - mll.mu[j], tb = xj - mlp.mu[j], tc = xj - mlq.mu[j];
                            qa = fma(ta * ta, mll.prec[j], qa);
                            qb = fma(tb * tb, mlp.prec[j], qb);
                            qc = fma(tc * tc, mlq.prec[j], qc);
                        }
                    }
                    nll = mll.logw[0] - 0.5 * qa;
                    nlp = mlp.logw[0] - 0.5 * qb;
                    nlq = mlq.logw[0] - 0.5 * qc;
                }
                const double lpn = log_p_t(nll, nlp, nlq, p.beta);
                const double lpo = log_p_t(oll, olp, olq, p.beta);
                const double log_a = (lpn + ref_corr_ct<TP>(q1, p.nu, dn)) - (lpo + ref_corr_ct<TP>(q0, p.nu, dn));
                const double u = accept_uniform(p.seed, gid, step);
                if (!PROPOSE) acc = log(u) < log_a;
                if (acc && !PROPOSE) {
                    if (ROW_OUT) {
                        regs_to_row<T, D>(myrow, v);
                    } else {
#pragma unroll
                        for (int j = 0; j < D; j++) soa_store<T>(ysr, ys_lane, ys_tile + (unsigned)j * ys_row, v[j]);
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
            const unsigned long long accmask = ROW_OUT ? __ballot(acc) : 0ULL;
            char* obase = PROPOSE ? reinterpret_cast<char*>(p.ys) + row0 * rowb : gbase;
            if (PAD) {
                if (accmask != 0ULL)
                    pad_tile_store_rows<T, D>(reinterpret_cast<T*>(obase), valid_bytes / (int64_t)sizeof(T), dr, magic, ldsrow, tile,
                                              lane, accmask);
            } else if (accmask != 0ULL) {
                tile_store_rows<16>(obase, valid_bytes, ROWB, LDSROW, tile, lane, accmask);
            }
        }
        wave_lds_sync();
    }
    if (!PROPOSE && (M == PCN_X_STEP || M == PCN_Y_STEP)) {
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

// gathers the caller's tables into the packed parameter block t (PTAB_SIZE + PTAB_BLK doubles), by one block of 256 threads
__device__ __forceinline__ void pcn_pack_block(const PcnDev& pd, double* __restrict__ t) {
    const int D = pd.dpad > pd.d ? pd.dpad : pd.d, dr = pd.d;  // tables of the D-dimensional kernel, identity beyond dr
    const int tri = D * (D + 1) / 2;
    for (int e = threadIdx.x; e < D * D; e += 256) {
        const int j = e / D, k = e - j * D;
        if (k <= j) {
            const bool in = j < dr;  // (k <= j < dr)
            t[j * (j + 1) / 2 + k] = in ? pd.L[j * dr + k] : (k == j ? 1.0 : 0.0);
            t[tri + j * (j + 1) / 2 + k] = in ? pd.Linv[j * dr + k] : (k == j ? 1.0 : 0.0);
        }
    }
    for (int e = threadIdx.x; e < D; e += 256) t[2 * tri + e] = e < dr ? pd.mu[e] : 0.0;
    if (D % 4 == 0) {  // the blocked copy of L (PTAB_BLK)
        double* tb = t + 2 * tri + D + 3 * PTAB_MIX(D);
        const int nblk = (D / 4) * (D / 4 + 1) / 2;
        for (int e = threadIdx.x; e < nblk * 16; e += 256) {
            const int b = e >> 4, kk = (e >> 2) & 3, r = e & 3;
            int g = 0;
            while ((g + 1) * (g + 2) / 2 <= b) g++;
            const int c = b - g * (g + 1) / 2, j = 4 * g + r, k = 4 * c + kk;
            tb[e] = k > j ? 0.0 : (j < dr ? pd.L[j * dr + k] : (k == j ? 1.0 : 0.0));
        }
    }
    double* m0 = t + 2 * tri + D;
    const MixDev* mixes[3] = {&pd.ll, &pd.lp, &pd.lq};
    for (int i = 0; i < 3; i++) {
        double* b = m0 + (size_t)i * PTAB_MIX(D);
        const int C = mixes[i]->C;
        for (int e = threadIdx.x; e < C; e += 256) b[e] = mixes[i]->logw[e];
        for (int e = threadIdx.x; e < C * D; e += 256) {
            b[ASMC_MAX_COMPONENTS + e] = mixes[i]->mu[e];
            b[ASMC_MAX_COMPONENTS * (1 + D) + e] = mixes[i]->prec[e];
        }
    }
}
