// asmc_nuts.hip — the NUTS mutation of the "blackjax_smc" sampler (reference src/aspire/samplers/smc/blackjax.py:229-277, its default
// algorithm): one independent chain per particle on the tempered log-target, a transition being a trajectory grown by doubling with
// multinomial sampling along it, iterative U-turn checkpoints and a divergence check.  Specification, counter layout and the state of
// the split path: include/asmc.h (asmc_nuts_*), DESIGN.md §3.18.
//
// Streams of particle gid at transition t under the mutation's key: the momenta are HMC's (normal_quad); the tree's own blocks have
// the counter {gid lo, gid hi, t, 0x60000000 | k}: k = 0 directions (bit j of word 0: doubling j goes forward), k = 1 + j the merge
// uniform of doubling j, k = 16 + m the sampling uniform of the leaf behind leapfrog step m of the transition.
//   k_nuts_mix       built-in densities (three diagonal Gaussian mixtures): whole transitions, several per launch, out of registers;
//                    the rows of a wave grow trees of different lengths, the wave stays converged: one leaf per pass of a bounded
//                    loop while any row builds, every state update under the row's predicate
//   k_nuts_begin / k_nuts_select / k_nuts_drift / (caller: gradients at z by torch.autograd) / k_nuts_leaf / k_nuts_merge /
//   k_nuts_finish    the same transition for any differentiable target, the population in lockstep, the state in device arrays
// The statistics of transition index t go to ctx->d_nuts[4 t ..]: moved rows, leapfrog steps, divergent rows, the integer sum of
// round(2^32 acceptance_sum / leaves); asmc_nuts_stats reads a chunk of them back once.
#include "asmc_hmc_dev.h"

#define NUTS_TAG 0x60000000u
#define NUTS_DIVERGENT 1
#define NUTS_TURNING 2

__device__ __forceinline__ void nuts_block(unsigned long long seed, unsigned long long gid, uint32_t t, uint32_t k, uint32_t w[4]) {
    philox4x32_10((uint32_t)gid, (uint32_t)(gid >> 32), t, NUTS_TAG | k, (uint32_t)seed, (uint32_t)(seed >> 32), w);
}
__device__ __forceinline__ double nuts_uniform(unsigned long long seed, unsigned long long gid, uint32_t t, uint32_t k) {
    uint32_t w[4];
    nuts_block(seed, gid, t, k, w);
    return u01_from_words(w[0], w[1]);
}
// log(exp(a) + exp(b)); a = -inf (an empty sub-tree) gives b
__device__ __forceinline__ double nuts_logaddexp(double a, double b) {
    const double m = fmax(a, b);
    return m == -INFINITY ? m : m + log1p(exp(-fabs(a - b)));
}
__device__ __forceinline__ unsigned long long nuts_acc_integer(double acc_sum, int leaves) {
    return leaves > 0 ? (unsigned long long)rint(4294967296.0 * (acc_sum / (double)leaves)) : 0ull;
}

// ---- fused NUTS on three diagonal Gaussian mixtures -----------------------------------------------------------------------------
// Row layout of asmc_hmc_dev.h with one quad per lane (NQ = 1): 2^LG lanes share a row.  Per row, in registers: the edge being
// extended A = (z, p, g), the other edge O, the tree's proposal P = (z, g), the sub-tree's proposal S, both momentum sums; "left" and
// "right" are only which of A / O is which (dirA), the whole-tree U-turn test being symmetric in them.  The checkpoints of the
// sub-tree U-turn tests (2 max_doublings vectors per row) live in the HBM workspace `ws`, one slab per BLOCK (not per row of the
// population): element e of checkpoint k, array w of this thread at ((blockIdx.x K + k) 2 + w) 4 + e) ASMC_BLOCK + threadIdx.x, so a
// wave's access is 512 contiguous bytes and a block re-reads what it wrote a few leaves ago.  One wave per SIMD (__launch_bounds__):
// the state and the target's working set need about 290 registers; at two waves per SIMD every instantiation spills to scratch.
#define NUTS_MAX_STEPS_PER_LAUNCH 256  // transitions whose statistics a block accumulates in LDS
#ifndef NUTS_WAVES
#define NUTS_WAVES 1  // waves per SIMD the kernel is built for (2 spills to scratch: a timing experiment only, tools/build_variant.sh)
#endif

struct NutsMixArgs {
    int max_doublings;
    double threshold;
    double* ws;
    int* info;  // [n, 4] (depth, leapfrog steps, flags, position) of the launch's last transition, or nullptr
};

template <int LG>
__global__ __launch_bounds__(ASMC_BLOCK, NUTS_WAVES) void k_nuts_mix(double* __restrict__ x, double* __restrict__ ll, double* __restrict__ lp,
                                                         double* __restrict__ lq, const HmcMixArgs a, const NutsMixArgs na,
                                                         unsigned long long* __restrict__ stats) {
    constexpr int TPR = 1 << LG, NC = 4, DPAD = NC * TPR, ROWS = ASMC_BLOCK >> LG;
    extern __shared__ __align__(16) double smem[];
    unsigned long long* s_cnt = reinterpret_cast<unsigned long long*>(smem);  // [n_steps][4] statistics of this block's rows
    double* t_ll = smem + 4 * a.n_steps;
    double* t_lp = t_ll + ASMC_MAX_COMPONENTS + 2 * a.ll.C * DPAD;
    double* t_lq = t_lp + ASMC_MAX_COMPONENTS + 2 * a.lp.C * DPAD;
    bm_d2* bmt = bm_lds();
    bm_tab_stage<ASMC_BLOCK>(bmt, a.bmtab);
    hmc_stage<DPAD>(t_ll, a.ll, a.d);
    hmc_stage<DPAD>(t_lp, a.lp, a.d);
    hmc_stage<DPAD>(t_lq, a.lq, a.d);
    for (int s = threadIdx.x; s < 4 * a.n_steps; s += ASMC_BLOCK) s_cnt[s] = 0ull;
    __syncthreads();

    const int lr = threadIdx.x & (TPR - 1), rib = threadIdx.x >> LG;
    const int K = na.max_doublings;
    const int max_leaves = (1 << K) - 1;
    double* const ck = na.ws + (size_t)blockIdx.x * (size_t)(2 * K * NC) * ASMC_BLOCK + threadIdx.x;  // + ((k 2 + w) 4 + e) ASMC_BLOCK
    double im[NC];  // diagonal of M^-1 (1 on the padding)
#pragma unroll
    for (int e = 0; e < NC; e++) {
        const int c = 4 * lr + e;
        im[e] = (c < a.d && a.minv != nullptr) ? a.minv[c] : 1.0;
    }
    const int64_t n_tiles = (a.n + ROWS - 1) / ROWS;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row = tile * ROWS + rib;
        const bool valid = row < a.n;
        const unsigned long long gid = a.gid0 + (unsigned long long)row;
        double PZ[NC], PG[NC];
#pragma unroll
        for (int e = 0; e < NC; e++) {
            const int c = 4 * lr + e;
            PZ[e] = (valid && c < a.d) ? x[row * a.d + c] : 0.0;
        }
        // the densities and the gradient at x are recomputed here, once per launch: the carried arrays are only written
        double vll, vlp, vlq;
        hmc_target<LG, 1>(t_ll, t_lp, t_lq, a, lr, PZ, vll, vlp, vlq, PG);
        bool moved = false;
        int depth = 0, m = 0, flags = 0, pos = 0;
#pragma unroll 1
        for (int s = 0; s < a.n_steps; s++) {
            const uint32_t t = a.step0 + (uint32_t)s;
            double AZ[NC], AP[NC], AG[NC], OZ[NC], OP[NC], OG[NC], SZ[NC], SG[NC], PS[NC], SPS[NC];
            {
                double z0, z1, z2, z3;
                normal_quad(a.seed, gid, t, (uint32_t)lr, bmt, z0, z1, z2, z3);
                const double z[4] = {z0, z1, z2, z3};
#pragma unroll
                for (int e = 0; e < NC; e++) {  // p ~ N(0, M); no momentum on the padding
                    AP[e] = 4 * lr + e < a.d ? z[e] / sqrt(im[e]) : 0.0;
                    AZ[e] = PZ[e];
                    AG[e] = PG[e];
                    OZ[e] = PZ[e];
                    OP[e] = AP[e];
                    OG[e] = PG[e];
                    SZ[e] = PZ[e];
                    SG[e] = PG[e];
                    PS[e] = AP[e];
                    SPS[e] = 0.0;
                }
            }
            const double lpt0 = log_p_t(vll, vlp, vlq, a.beta);
            const double E0 = hmc_kinetic<LG, 1>(AP, im) - lpt0;
            bool act = valid && lpt0 > -INFINITY;  // a start in a hole of the target: the row stays, no step
            uint32_t dirw;
            {
                uint32_t w[4];
                nuts_block(a.seed, gid, t, 0u, w);
                dirw = w[0];
            }
            double tree_lw = 0.0, sub_lw = -INFINITY, accs = 0.0, sll = vll, slp = vlp, slq = vlq;
            int i = 0, leaves = 0, nA = 0, nO = 0, dirA = 1, spos = 0;
            depth = 0;
            m = 0;
            flags = 0;
            pos = 0;
#pragma unroll 1
            for (int it = 0; it < max_leaves && __any(act); it++) {
                // a new doubling: the edge on the drawn side becomes A, the sub-tree is empty
                const bool fresh = act && i == 0;
                const int v = ((dirw >> depth) & 1u) ? 1 : -1;
                const bool sw = fresh && v != dirA;
#pragma unroll
                for (int e = 0; e < NC; e++) {
                    const double tz = AZ[e], tp = AP[e], tg = AG[e];
                    AZ[e] = sw ? OZ[e] : tz;
                    AP[e] = sw ? OP[e] : tp;
                    AG[e] = sw ? OG[e] : tg;
                    OZ[e] = sw ? tz : OZ[e];
                    OP[e] = sw ? tp : OP[e];
                    OG[e] = sw ? tg : OG[e];
                    SPS[e] = fresh ? 0.0 : SPS[e];
                }
                if (sw) {
                    const int tn = nA;
                    nA = nO;
                    nO = tn;
                    dirA = v;
                }
                sub_lw = fresh ? -INFINITY : sub_lw;
                // one velocity-Verlet step of size dirA eps from A
                const double fe = dirA > 0 ? a.eps : -a.eps, he = 0.5 * fe;
                double zn[NC], pn[NC], gn[NC];
#pragma unroll
                for (int e = 0; e < NC; e++) {
                    pn[e] = AP[e] + he * AG[e];
                    zn[e] = AZ[e] + fe * (im[e] * pn[e]);
                }
                double nll, nlp, nlq;
                hmc_target<LG, 1>(t_ll, t_lp, t_lq, a, lr, zn, nll, nlp, nlq, gn);
#pragma unroll
                for (int e = 0; e < NC; e++) pn[e] = pn[e] + he * gn[e];
                const double delta = (hmc_kinetic<LG, 1>(pn, im) - log_p_t(nll, nlp, nlq, a.beta)) - E0;
                const double u_leaf = nuts_uniform(a.seed, gid, t, 16u + (uint32_t)m);
                const bool div = act && !(delta <= na.threshold);  // (a NaN counts as over)
                const bool ok = act && !div;
                const double lw = -delta;
                const double nw = nuts_logaddexp(sub_lw, lw);
                const bool take = ok && (i == 0 || u_leaf < exp(lw - nw));
#pragma unroll
                for (int e = 0; e < NC; e++) {
                    AZ[e] = act ? zn[e] : AZ[e];
                    AP[e] = act ? pn[e] : AP[e];
                    AG[e] = act ? gn[e] : AG[e];
                    SZ[e] = take ? zn[e] : SZ[e];
                    SG[e] = take ? gn[e] : SG[e];
                    SPS[e] = ok ? SPS[e] + pn[e] : SPS[e];
                }
                m += act ? 1 : 0;
                accs += ok ? fmin(1.0, exp(lw)) : 0.0;
                leaves += ok ? 1 : 0;
                sll = take ? nll : sll;
                slp = take ? nlp : slp;
                slq = take ? nlq : slq;
                spos = take ? dirA * (nA + i + 1) : spos;
                sub_lw = ok ? nw : sub_lw;
                // the sub-tree's U-turn checkpoints: an even leaf opens one, an odd leaf closes as many as it has trailing one bits
                const int top = __popc((unsigned)i >> 1);
                const bool odd = (i & 1) != 0;
                if (ok && !odd) {
#pragma unroll
                    for (int e = 0; e < NC; e++) {
                        ck[(size_t)((top * 2 + 0) * NC + e) * ASMC_BLOCK] = pn[e];
                        ck[(size_t)((top * 2 + 1) * NC + e) * ASMC_BLOCK] = SPS[e];
                    }
                }
                const int ones = odd ? __ffs(~i) - 1 : 0;
                bool turn = false;
#pragma unroll 1
                for (int c = 0; c < K && __any(ok && c < ones); c++) {
                    const bool chk = ok && c < ones;
                    const int k = chk ? top - c : 0;
                    double d1 = 0.0, d2 = 0.0;
#pragma unroll
                    for (int e = 0; e < NC; e++) {
                        const double cp = chk ? ck[(size_t)((k * 2 + 0) * NC + e) * ASMC_BLOCK] : 0.0;
                        const double cs = chk ? ck[(size_t)((k * 2 + 1) * NC + e) * ASMC_BLOCK] : 0.0;
                        const double ms = im[e] * (SPS[e] - cs + cp);
                        d1 = fma(cp, ms, d1);
                        d2 = fma(pn[e], ms, d2);
                    }
                    d1 = hmc_row_sum<LG>(d1);
                    d2 = hmc_row_sum<LG>(d2);
                    turn = turn || (chk && (d1 <= 0.0 || d2 <= 0.0));
                }
                // the sub-tree is complete: merge it, then the whole tree's U-turn test (symmetric in the two edges).  Once per 2^depth
                // leaves of a row, so the whole block runs only when some row of the wave is there
                const bool full = ok && !turn && i == (1 << depth) - 1;
                bool whole_turn = false;
                if (__any(full)) {
                    double w1 = 0.0, w2 = 0.0;
#pragma unroll
                    for (int e = 0; e < NC; e++) {
                        const double ms = im[e] * (PS[e] + SPS[e]);
                        w1 = fma(AP[e], ms, w1);
                        w2 = fma(OP[e], ms, w2);
                    }
                    w1 = hmc_row_sum<LG>(w1);
                    w2 = hmc_row_sum<LG>(w2);
                    whole_turn = full && (w1 <= 0.0 || w2 <= 0.0);
                    const bool adopt = full && nuts_uniform(a.seed, gid, t, 1u + (uint32_t)depth) < exp(fmin(0.0, sub_lw - tree_lw));
#pragma unroll
                    for (int e = 0; e < NC; e++) {
                        PZ[e] = adopt ? SZ[e] : PZ[e];
                        PG[e] = adopt ? SG[e] : PG[e];
                        PS[e] = full ? PS[e] + SPS[e] : PS[e];
                    }
                    vll = adopt ? sll : vll;
                    vlp = adopt ? slp : vlp;
                    vlq = adopt ? slq : vlq;
                    pos = adopt ? spos : pos;
                    const double merged_lw = nuts_logaddexp(tree_lw, sub_lw);
                    tree_lw = full ? merged_lw : tree_lw;
                    nA += full ? (1 << depth) : 0;
                    depth += full ? 1 : 0;
                }
                flags |= (div ? NUTS_DIVERGENT : 0) | ((turn || whole_turn) ? NUTS_TURNING : 0);
                i = full ? 0 : (ok ? i + 1 : i);
                act = ok && !turn && !whole_turn && depth < K;
            }
            const bool mv = valid && pos != 0;
            moved = moved || mv;
            const unsigned long long bm = __ballot(mv && lr == 0), bd = __ballot(valid && (flags & NUTS_DIVERGENT) && lr == 0);
            if ((threadIdx.x & (ASMC_WAVE - 1)) == 0) {
                if (bm != 0ull) atomicAdd(&s_cnt[4 * s + 0], (unsigned long long)__popcll(bm));
                if (bd != 0ull) atomicAdd(&s_cnt[4 * s + 2], (unsigned long long)__popcll(bd));
            }
            if (valid && lr == 0 && m > 0) {
                atomicAdd(&s_cnt[4 * s + 1], (unsigned long long)m);
                atomicAdd(&s_cnt[4 * s + 3], nuts_acc_integer(accs, leaves));
            }
        }
        if (moved) {
#pragma unroll
            for (int e = 0; e < NC; e++) {
                const int c = 4 * lr + e;
                if (c < a.d) x[row * a.d + c] = PZ[e];
            }
            if (lr == 0) {
                ll[row] = vll;
                lp[row] = vlp;
                lq[row] = vlq;
            }
        }
        if (na.info != nullptr && valid && lr == 0) {
            int* o = na.info + row * 4;
            o[0] = depth;
            o[1] = m;
            o[2] = flags;
            o[3] = pos;
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < 4 * a.n_steps; s += ASMC_BLOCK)
        if (s_cnt[s] != 0ull) atomicAdd(stats + s, s_cnt[s]);
}

// ---- split path -----------------------------------------------------------------------------------------------------------------
// The state of a mutation's trees (asmc_nuts_state, include/asmc.h): vec [slots][n][d], sc [slots][n], ist [slots][n].  One thread
// per row; the population is in lockstep, so leaf index and doubling are launch arguments.
enum { NV_ZL, NV_PL, NV_GL, NV_ZR, NV_PR, NV_GR, NV_ZC, NV_PC, NV_GC, NV_ZS, NV_GS, NV_ZP, NV_GP, NV_PSUM, NV_SPSUM, NV_CK };
enum { NS_E0, NS_TREE_LW, NS_SUB_LW, NS_ACCS, NS_DP, NS_DS = NS_DP + 3, NS_COUNT = NS_DS + 3 };
enum { NI_DEPTH, NI_STEPS, NI_LEAVES, NI_FLAGS, NI_POS, NI_SPOS, NI_NL, NI_NR, NI_V, NI_DIRW, NI_BUILDING, NI_ALIVE, NI_COUNT };
static_assert(NV_ZC == ASMC_NUTS_VEC_Z && NV_ZP == ASMC_NUTS_VEC_POINT && NV_GP == ASMC_NUTS_VEC_GRAD && NV_CK == ASMC_NUTS_VEC_FIXED &&
                  NS_DP == ASMC_NUTS_SC_DENSITIES && NS_COUNT == ASMC_NUTS_SC_SLOTS && NI_COUNT == ASMC_NUTS_INT_SLOTS,
              "asmc.h's slot numbers");

struct NutsDev {
    int64_t n;
    int d, K;
    double* vec;
    double* sc;
    int* ist;
    const double* minv;
    double eps, beta, thr;
    __device__ __forceinline__ double* V(int slot, int64_t i) const { return vec + ((size_t)slot * n + i) * d; }
    __device__ __forceinline__ double& S(int slot, int64_t i) const { return sc[(size_t)slot * n + i]; }
    __device__ __forceinline__ int& I(int slot, int64_t i) const { return ist[(size_t)slot * n + i]; }
    __device__ __forceinline__ double im(int j) const { return minv != nullptr ? minv[j] : 1.0; }
};

__device__ __forceinline__ void nuts_copy(double* __restrict__ dst, const double* __restrict__ src, int d) {
    for (int j = 0; j < d; j++) dst[j] = src[j];
}
// turning(a, b, s) with s = s1 - s2 + s3 (s2, s3 may be nullptr)
__device__ __forceinline__ bool nuts_turning(const NutsDev& a, const double* pa, const double* pb, const double* s1, const double* s2,
                                             const double* s3) {
    double da = 0.0, db = 0.0;
    for (int j = 0; j < a.d; j++) {
        double s = s1[j];
        if (s2 != nullptr) s = s - s2[j] + s3[j];
        const double ms = a.im(j) * s;
        da = fma(pa[j], ms, da);
        db = fma(pb[j], ms, db);
    }
    return da <= 0.0 || db <= 0.0;
}

__global__ __launch_bounds__(ASMC_BLOCK) void k_nuts_begin(const NutsDev a, unsigned long long seed, unsigned long long gid0, uint32_t step,
                                                           const double* __restrict__ bmtab) {
    bm_d2* bmt = bm_lds();
    bm_tab_stage<ASMC_BLOCK>(bmt, bmtab);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const unsigned long long gid = gid0 + (unsigned long long)i;
    double* p0 = a.V(NV_PC, i);
    double ke = 0.0;
    for (int q = 0; 4 * q < a.d; q++) {
        double z[4];
        normal_quad(seed, gid, step, (uint32_t)q, bmt, z[0], z[1], z[2], z[3]);
        for (int e = 0; e < 4 && 4 * q + e < a.d; e++) {
            const int j = 4 * q + e;
            const double p = z[e] / sqrt(a.im(j));
            p0[j] = p;
            ke = fma(a.im(j) * p, p, ke);
        }
    }
    const double lpt = log_p_t(a.S(NS_DP, i), a.S(NS_DP + 1, i), a.S(NS_DP + 2, i), a.beta);
    a.S(NS_E0, i) = 0.5 * ke - lpt;
    a.S(NS_TREE_LW, i) = 0.0;
    a.S(NS_ACCS, i) = 0.0;
    const double *zp = a.V(NV_ZP, i), *gp = a.V(NV_GP, i);
    nuts_copy(a.V(NV_ZL, i), zp, a.d);
    nuts_copy(a.V(NV_ZR, i), zp, a.d);
    nuts_copy(a.V(NV_ZC, i), zp, a.d);
    nuts_copy(a.V(NV_GL, i), gp, a.d);
    nuts_copy(a.V(NV_GR, i), gp, a.d);
    nuts_copy(a.V(NV_GC, i), gp, a.d);
    nuts_copy(a.V(NV_PL, i), p0, a.d);
    nuts_copy(a.V(NV_PR, i), p0, a.d);
    nuts_copy(a.V(NV_PSUM, i), p0, a.d);
    for (int s = NI_DEPTH; s <= NI_NR; s++) a.I(s, i) = 0;
    uint32_t w[4];
    nuts_block(seed, gid, step, 0u, w);
    a.I(NI_DIRW, i) = (int)w[0];
    a.I(NI_BUILDING, i) = lpt > -INFINITY;
    a.I(NI_ALIVE, i) = 0;
}

__global__ __launch_bounds__(ASMC_BLOCK) void k_nuts_select(const NutsDev a) {
    const int64_t i = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const int b = a.I(NI_BUILDING, i);
    a.I(NI_ALIVE, i) = b;
    if (!b) return;
    const bool fwd = (((uint32_t)a.I(NI_DIRW, i) >> a.I(NI_DEPTH, i)) & 1u) != 0u;
    a.I(NI_V, i) = fwd ? 1 : -1;
    nuts_copy(a.V(NV_ZC, i), a.V(fwd ? NV_ZR : NV_ZL, i), a.d);
    nuts_copy(a.V(NV_PC, i), a.V(fwd ? NV_PR : NV_PL, i), a.d);
    nuts_copy(a.V(NV_GC, i), a.V(fwd ? NV_GR : NV_GL, i), a.d);
    a.S(NS_SUB_LW, i) = -INFINITY;
    double* sps = a.V(NV_SPSUM, i);
    for (int j = 0; j < a.d; j++) sps[j] = 0.0;
}

__global__ __launch_bounds__(ASMC_BLOCK) void k_nuts_drift(const NutsDev a) {
    const int64_t i = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x;
    if (i >= a.n || !a.I(NI_ALIVE, i)) return;
    const double fe = a.I(NI_V, i) > 0 ? a.eps : -a.eps, he = 0.5 * fe;
    double *z = a.V(NV_ZC, i), *p = a.V(NV_PC, i);
    const double* g = a.V(NV_GC, i);
    for (int j = 0; j < a.d; j++) {
        const double pj = p[j] + he * g[j];
        p[j] = pj;
        z[j] = z[j] + fe * (a.im(j) * pj);
    }
}

__global__ __launch_bounds__(ASMC_BLOCK) void k_nuts_leaf(const NutsDev a, int leaf, const double* __restrict__ g_new,
                                                          const double* __restrict__ ll_new, const double* __restrict__ lp_new,
                                                          const double* __restrict__ lq_new, unsigned long long seed, unsigned long long gid0,
                                                          uint32_t step) {
    const int64_t i = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x;
    if (i >= a.n || !a.I(NI_ALIVE, i)) return;
    const int v = a.I(NI_V, i);
    const double he = 0.5 * (v > 0 ? a.eps : -a.eps);
    double *p = a.V(NV_PC, i), *g = a.V(NV_GC, i), *z = a.V(NV_ZC, i);
    double ke = 0.0;
    for (int j = 0; j < a.d; j++) {
        const double gj = g_new[i * a.d + j];
        const double pj = p[j] + he * gj;
        p[j] = pj;
        g[j] = gj;
        ke = fma(a.im(j) * pj, pj, ke);
    }
    const double delta = (0.5 * ke - log_p_t(ll_new[i], lp_new[i], lq_new[i], a.beta)) - a.S(NS_E0, i);
    const int m = a.I(NI_STEPS, i);
    a.I(NI_STEPS, i) = m + 1;
    int ended = 0;
    if (!(delta <= a.thr)) {
        ended = NUTS_DIVERGENT;
    } else {
        const double lw = -delta, sub = a.S(NS_SUB_LW, i);
        a.S(NS_ACCS, i) += fmin(1.0, exp(lw));
        a.I(NI_LEAVES, i) += 1;
        const double nw = nuts_logaddexp(sub, lw);
        if (leaf == 0 || nuts_uniform(seed, gid0 + (unsigned long long)i, step, 16u + (uint32_t)m) < exp(lw - nw)) {
            nuts_copy(a.V(NV_ZS, i), z, a.d);
            nuts_copy(a.V(NV_GS, i), g, a.d);
            a.S(NS_DS, i) = ll_new[i];
            a.S(NS_DS + 1, i) = lp_new[i];
            a.S(NS_DS + 2, i) = lq_new[i];
            a.I(NI_SPOS, i) = v * (a.I(v > 0 ? NI_NR : NI_NL, i) + leaf + 1);
        }
        a.S(NS_SUB_LW, i) = nw;
        double* sps = a.V(NV_SPSUM, i);
        for (int j = 0; j < a.d; j++) sps[j] += p[j];
        const int top = __popc((unsigned)leaf >> 1);
        if (!(leaf & 1)) {
            nuts_copy(a.V(NV_CK + top, i), p, a.d);
            nuts_copy(a.V(NV_CK + a.K + top, i), sps, a.d);
        } else {
            const int ones = __ffs(~leaf) - 1;
            for (int k = top; k > top - ones; k--)
                if (nuts_turning(a, a.V(NV_CK + k, i), p, sps, a.V(NV_CK + a.K + k, i), a.V(NV_CK + k, i))) ended = NUTS_TURNING;
        }
    }
    if (ended) {
        a.I(NI_FLAGS, i) |= ended;
        a.I(NI_ALIVE, i) = 0;
        a.I(NI_BUILDING, i) = 0;
        nuts_copy(z, a.V(NV_ZP, i), a.d);  // a finite point for the gradient launches that still see the row
    }
}

__global__ __launch_bounds__(ASMC_BLOCK) void k_nuts_merge(const NutsDev a, int doubling, unsigned long long seed, unsigned long long gid0,
                                                           uint32_t step, unsigned long long* __restrict__ building) {
    const int64_t i = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x;
    bool still = false;
    if (i < a.n && a.I(NI_ALIVE, i)) {
        const bool fwd = a.I(NI_V, i) > 0;
        nuts_copy(a.V(fwd ? NV_ZR : NV_ZL, i), a.V(NV_ZC, i), a.d);
        nuts_copy(a.V(fwd ? NV_PR : NV_PL, i), a.V(NV_PC, i), a.d);
        nuts_copy(a.V(fwd ? NV_GR : NV_GL, i), a.V(NV_GC, i), a.d);
        a.I(fwd ? NI_NR : NI_NL, i) += 1 << doubling;
        const double sub = a.S(NS_SUB_LW, i), tree = a.S(NS_TREE_LW, i);
        if (nuts_uniform(seed, gid0 + (unsigned long long)i, step, 1u + (uint32_t)doubling) < exp(fmin(0.0, sub - tree))) {
            nuts_copy(a.V(NV_ZP, i), a.V(NV_ZS, i), a.d);
            nuts_copy(a.V(NV_GP, i), a.V(NV_GS, i), a.d);
            for (int k = 0; k < 3; k++) a.S(NS_DP + k, i) = a.S(NS_DS + k, i);
            a.I(NI_POS, i) = a.I(NI_SPOS, i);
        }
        a.S(NS_TREE_LW, i) = nuts_logaddexp(tree, sub);
        double* ps = a.V(NV_PSUM, i);
        const double* sps = a.V(NV_SPSUM, i);
        for (int j = 0; j < a.d; j++) ps[j] += sps[j];
        const int depth = a.I(NI_DEPTH, i) + 1;
        a.I(NI_DEPTH, i) = depth;
        const bool turn = nuts_turning(a, a.V(NV_PL, i), a.V(NV_PR, i), ps, nullptr, nullptr);
        if (turn) a.I(NI_FLAGS, i) |= NUTS_TURNING;
        still = !turn && depth < a.K;
        a.I(NI_BUILDING, i) = still;
        a.I(NI_ALIVE, i) = 0;
        nuts_copy(a.V(NV_ZC, i), a.V(NV_ZP, i), a.d);
    }
    const unsigned long long b = __ballot(still);
    if ((threadIdx.x & (ASMC_WAVE - 1)) == 0 && b != 0ull) atomicAdd(building, (unsigned long long)__popcll(b));
}

template <typename T>
__global__ __launch_bounds__(ASMC_BLOCK) void k_nuts_finish(const NutsDev a, T* __restrict__ x, double* __restrict__ ll, double* __restrict__ lp,
                                                            double* __restrict__ lq, int* __restrict__ info,
                                                            unsigned long long* __restrict__ stats) {
    const int64_t i = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x;
    const bool valid = i < a.n;
    bool mv = false, dv = false;
    unsigned long long steps = 0ull, q = 0ull;
    if (valid) {
        const int pos = a.I(NI_POS, i), flags = a.I(NI_FLAGS, i), m = a.I(NI_STEPS, i);
        mv = pos != 0;
        dv = (flags & NUTS_DIVERGENT) != 0;
        steps = (unsigned long long)m;
        q = nuts_acc_integer(a.S(NS_ACCS, i), a.I(NI_LEAVES, i));
        if (mv) {
            const double* zp = a.V(NV_ZP, i);
            for (int j = 0; j < a.d; j++) x[i * a.d + j] = (T)zp[j];
            ll[i] = a.S(NS_DP, i);
            lp[i] = a.S(NS_DP + 1, i);
            lq[i] = a.S(NS_DP + 2, i);
        }
        if (info != nullptr) {
            info[4 * i + 0] = a.I(NI_DEPTH, i);
            info[4 * i + 1] = m;
            info[4 * i + 2] = flags;
            info[4 * i + 3] = pos;
        }
    }
    const unsigned long long bm = __ballot(mv), bd = __ballot(dv);
    steps = (unsigned long long)wave_sum_ll((long long)steps);
    q = (unsigned long long)wave_sum_ll((long long)q);
    if ((threadIdx.x & (ASMC_WAVE - 1)) == 0) {
        if (bm != 0ull) atomicAdd(stats + 0, (unsigned long long)__popcll(bm));
        if (steps != 0ull) atomicAdd(stats + 1, steps);
        if (bd != 0ull) atomicAdd(stats + 2, (unsigned long long)__popcll(bd));
        if (q != 0ull) atomicAdd(stats + 3, q);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
static int nuts_ws_reserve(asmc_ctx* ctx, size_t bytes, hipStream_t st) {
    if (ctx->nuts_ws_bytes >= bytes) return ASMC_OK;
    ASMC_HIP(hipStreamSynchronize(st));  // a launch in flight may still use the old workspace
    if (ctx->d_nuts_ws) ASMC_HIP(hipFree(ctx->d_nuts_ws));
    ctx->d_nuts_ws = nullptr;
    ctx->nuts_ws_bytes = 0;
    ASMC_HIP(hipMalloc((void**)&ctx->d_nuts_ws, bytes));
    ctx->nuts_ws_bytes = bytes;
    return ASMC_OK;
}

template <int LG>
static int nuts_mix_launch(asmc_ctx* ctx, double* x, double* ll, double* lp, double* lq, const HmcMixArgs& a, NutsMixArgs na, int max_blocks,
                           unsigned long long* stats, hipStream_t st) {
    constexpr int DPAD = 4 << LG, ROWS = ASMC_BLOCK >> LG;
    const size_t lds = sizeof(double) * (4 * a.n_steps + 3 * ASMC_MAX_COMPONENTS + 2 * DPAD * (a.ll.C + a.lp.C + a.lq.C));
    const int64_t tiles = (a.n + ROWS - 1) / ROWS;
    const int64_t cap = max_blocks > 0 ? max_blocks : (int64_t)ctx->num_cu * NUTS_WAVES;  // one block per CU is resident (registers)
    const int grid = (int)(tiles < cap ? tiles : cap);
    const int rc = nuts_ws_reserve(ctx, sizeof(double) * (size_t)grid * 2 * na.max_doublings * 4 * ASMC_BLOCK, st);
    if (rc) return rc;
    na.ws = ctx->d_nuts_ws;
    ASMC_LAUNCH(ctx, st, "k_nuts_mix", (k_nuts_mix<LG>), dim3(grid), dim3(ASMC_BLOCK), lds, st, x, ll, lp, lq, a, na, stats);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

static int nuts_state_dev(const asmc_nuts_state* s, NutsDev& a, const char* who) {
    if (s == nullptr || !(s->n >= 1 && s->n < (1LL << 31) && s->d > 0 && s->d <= ASMC_MAX_DIMS) ||
        !(s->max_doublings >= 1 && s->max_doublings <= ASMC_NUTS_MAX_DOUBLINGS) || !s->vec_dev || !s->sc_dev || !s->ist_dev ||
        !(s->step_size > 0.0)) {
        asmc_set_error("%s: bad state (1 <= n < 2^31, 0 < d <= ASMC_MAX_DIMS, 1 <= max_doublings <= 10, arrays, step_size > 0)", who);
        return ASMC_ERR_ARG;
    }
    a.n = s->n;
    a.d = s->d;
    a.K = s->max_doublings;
    a.vec = s->vec_dev;
    a.sc = s->sc_dev;
    a.ist = s->ist_dev;
    a.minv = s->minv_dev;
    a.eps = s->step_size;
    a.beta = s->beta;
    a.thr = s->threshold;
    return ASMC_OK;
}

#define NUTS_SPLIT_PROLOGUE()                            \
    ASMC_REQUIRE(ctx != nullptr, "null context");        \
    NutsDev a;                                           \
    {                                                    \
        const int rc = nuts_state_dev(state, a, __func__); \
        if (rc) return rc;                               \
    }                                                    \
    hipStream_t st = as_stream(stream);                  \
    const int grid = (int)((a.n + ASMC_BLOCK - 1) / ASMC_BLOCK)

extern "C" {

int asmc_nuts_mix(asmc_ctx* ctx, int64_t n, int d, void* x, double* ll, double* lp, double* lq, double beta,
                  const asmc_mixture* log_likelihood, const asmc_mixture* log_prior, const asmc_mixture* log_q, const double* minv,
                  double step_size, int max_doublings, double threshold, uint64_t seed, uint64_t gid0, uint32_t step0, int n_steps, int t0,
                  int max_blocks, int* info_out, asmc_stream stream) {
    ASMC_REQUIRE(ctx != nullptr && n >= 1 && n < (1LL << 31) && d > 0 && d <= HMC_FUSED_MAX_D, "bad arguments (ctx, 1 <= n < 2^31, 0 < d <= 128)");
    ASMC_REQUIRE(x && ll && lp && lq && log_likelihood && log_prior && log_q, "null pointer");
    ASMC_REQUIRE(n_steps >= 1 && n_steps <= NUTS_MAX_STEPS_PER_LAUNCH && t0 >= 0 && t0 + n_steps <= ASMC_MAX_PCN_STEPS,
                 "1 <= n_steps <= 256 per launch, t0 + n_steps <= 2048");
    ASMC_REQUIRE(max_doublings >= 1 && max_doublings <= ASMC_NUTS_MAX_DOUBLINGS, "max_num_doublings must be in 1 .. 10");
    ASMC_REQUIRE(step_size > 0.0 && max_blocks >= 0, "step_size must be positive, max_blocks >= 0");
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
    a.step0 = step0;
    a.eps = step_size;
    a.beta = beta;
    a.seed = seed;
    a.gid0 = gid0;
    a.minv = minv;
    a.bmtab = ctx->d_bmtab;
    NutsMixArgs na;
    na.max_doublings = max_doublings;
    na.threshold = threshold;
    na.ws = nullptr;
    na.info = info_out;
    hipStream_t st = as_stream(stream);
    unsigned long long* stats = ctx->d_nuts + 4 * t0;
    ASMC_HIP(hipMemsetAsync(stats, 0, sizeof(unsigned long long) * 4 * n_steps, st));
    double* xd = (double*)x;
    if (d <= 4) return nuts_mix_launch<0>(ctx, xd, ll, lp, lq, a, na, max_blocks, stats, st);
    if (d <= 8) return nuts_mix_launch<1>(ctx, xd, ll, lp, lq, a, na, max_blocks, stats, st);
    if (d <= 16) return nuts_mix_launch<2>(ctx, xd, ll, lp, lq, a, na, max_blocks, stats, st);
    if (d <= 32) return nuts_mix_launch<3>(ctx, xd, ll, lp, lq, a, na, max_blocks, stats, st);
    if (d <= 64) return nuts_mix_launch<4>(ctx, xd, ll, lp, lq, a, na, max_blocks, stats, st);
    return nuts_mix_launch<5>(ctx, xd, ll, lp, lq, a, na, max_blocks, stats, st);
}

int asmc_nuts_stats(asmc_ctx* ctx, int n_steps, int64_t* stats_host, asmc_stream stream) {
    ASMC_REQUIRE(ctx && stats_host, "null pointer");
    ASMC_REQUIRE(n_steps >= 1 && n_steps <= ASMC_MAX_PCN_STEPS, "n_steps out of range");
    hipStream_t st = as_stream(stream);
    unsigned long long* h = reinterpret_cast<unsigned long long*>(ctx->h_pinned);
    ASMC_HIP(hipStreamSynchronize(st));  // pinned staging may still be in flight
    ASMC_HIP(hipMemcpyAsync(h, ctx->d_nuts, sizeof(unsigned long long) * 4 * n_steps, hipMemcpyDeviceToHost, st));
    ASMC_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < 4 * n_steps; i++) stats_host[i] = (int64_t)h[i];
    return ASMC_OK;
}

int asmc_nuts_begin(asmc_ctx* ctx, const asmc_nuts_state* state, uint64_t seed, uint64_t gid0, uint32_t step, asmc_stream stream) {
    NUTS_SPLIT_PROLOGUE();
    ASMC_LAUNCH(ctx, st, "k_nuts_begin", k_nuts_begin, dim3(grid), dim3(ASMC_BLOCK), 0, st, a, seed, gid0, step, ctx->d_bmtab);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int asmc_nuts_select(asmc_ctx* ctx, const asmc_nuts_state* state, asmc_stream stream) {
    NUTS_SPLIT_PROLOGUE();
    ASMC_LAUNCH(ctx, st, "k_nuts_select", k_nuts_select, dim3(grid), dim3(ASMC_BLOCK), 0, st, a);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int asmc_nuts_drift(asmc_ctx* ctx, const asmc_nuts_state* state, asmc_stream stream) {
    NUTS_SPLIT_PROLOGUE();
    ASMC_LAUNCH(ctx, st, "k_nuts_drift", k_nuts_drift, dim3(grid), dim3(ASMC_BLOCK), 0, st, a);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int asmc_nuts_leaf(asmc_ctx* ctx, const asmc_nuts_state* state, int leaf, const double* g_new, const double* ll_new, const double* lp_new,
                   const double* lq_new, uint64_t seed, uint64_t gid0, uint32_t step, asmc_stream stream) {
    NUTS_SPLIT_PROLOGUE();
    ASMC_REQUIRE(g_new && ll_new && lp_new && lq_new, "null pointer");
    ASMC_REQUIRE(leaf >= 0 && leaf < (1 << (a.K - 1)), "leaf index out of range");
    ASMC_LAUNCH(ctx, st, "k_nuts_leaf", k_nuts_leaf, dim3(grid), dim3(ASMC_BLOCK), 0, st, a, leaf, g_new, ll_new, lp_new, lq_new, seed, gid0,
                step);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int asmc_nuts_merge(asmc_ctx* ctx, const asmc_nuts_state* state, int doubling, uint64_t seed, uint64_t gid0, uint32_t step,
                    int64_t* building_host, asmc_stream stream) {
    NUTS_SPLIT_PROLOGUE();
    ASMC_REQUIRE(building_host != nullptr, "null pointer");
    ASMC_REQUIRE(doubling >= 0 && doubling < a.K, "doubling out of range");
    unsigned long long* cell = ctx->d_nuts + 4 * ASMC_MAX_PCN_STEPS;
    unsigned long long* h = reinterpret_cast<unsigned long long*>(ctx->h_pinned);
    ASMC_HIP(hipMemsetAsync(cell, 0, sizeof(unsigned long long), st));
    ASMC_LAUNCH(ctx, st, "k_nuts_merge", k_nuts_merge, dim3(grid), dim3(ASMC_BLOCK), 0, st, a, doubling, seed, gid0, step, cell);
    ASMC_LAUNCH_CHECK();
    ASMC_HIP(hipMemcpyAsync(h, cell, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    ASMC_HIP(hipStreamSynchronize(st));
    *building_host = (int64_t)h[0];
    return ASMC_OK;
}

int asmc_nuts_finish(asmc_ctx* ctx, const asmc_nuts_state* state, int x_dtype, void* x, double* ll, double* lp, double* lq, int t,
                     int* info_out, asmc_stream stream) {
    NUTS_SPLIT_PROLOGUE();
    ASMC_REQUIRE(x_dtype == ASMC_F64 || x_dtype == ASMC_F32, "bad x_dtype");
    ASMC_REQUIRE(x && ll && lp && lq, "null pointer");
    ASMC_REQUIRE(t >= 0 && t < ASMC_MAX_PCN_STEPS, "step index out of range");
    unsigned long long* stats = ctx->d_nuts + 4 * t;
    ASMC_HIP(hipMemsetAsync(stats, 0, sizeof(unsigned long long) * 4, st));
    if (x_dtype == ASMC_F64)
        ASMC_LAUNCH(ctx, st, "k_nuts_finish", k_nuts_finish<double>, dim3(grid), dim3(ASMC_BLOCK), 0, st, a, (double*)x, ll, lp, lq, info_out,
                    stats);
    else
        ASMC_LAUNCH(ctx, st, "k_nuts_finish", k_nuts_finish<float>, dim3(grid), dim3(ASMC_BLOCK), 0, st, a, (float*)x, ll, lp, lq, info_out,
                    stats);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

}  // extern "C"
