// asmc_search_dev.h — the device half of the adaptive-temperature search (the reduction of a round's partial records, the round tail on a block-local or a global state record, the merge of
// the ranks' records of a sharded search) with the few host helpers that go with the state record.
// Included by asmc_search.hip (k_bis_sums, k_bis_decide, the one-chain sharded passes) and asmc_is_weights.hip (k_is_weights);
// the plain passes (asmc_weights.hip) do not see it - what they share with the search is asmc_weights_dev.h.  The decisions themselves are plain C++: asmc_bisect.h.
#pragma once
#include <stdlib.h>

#include "asmc_common.h"
#include "asmc_bisect.h"
#include "asmc_weights_dev.h"

// ---------------------------------------------------------------------------------------------
// Device-side k-ary bisection (smc/base.py:167-186): the whole adaptive-beta search runs as a chain of
// launches without host round trips.  State: BIS_STATE_LEN doubles in ctx->d_small + DS_BISECT (asmc_scratch.h), laid out
// by the BIS_* enum of asmc_bisect.h.
#define BIS_LEVELS 4
#define BIS_NODES 15

__device__ __forceinline__ double ess_over_n(double m, double S1, double S2, double logN, double N) {
    // the host's smc_math.ess (utils.py:510-512 on samples.py:1244-1249), same operation order
    const double c = (m + log(S1)) - logN;
    const double mp = m + c;
    const double l1 = mp + log(S1);
    const double l2 = mp * 2.0 + log(S2);
    return exp(l1 * 2.0 - l2) / N;
}

struct BisInit {
    double beta0, target, tol, logN, N;
    double plain;  // 1: no prediction windows (ASMC_BISECT_PLAIN: the 16-ary search of rounds 1-2, for comparison)
};
static double bis_plain_mode() {
    static const double v = getenv("ASMC_BISECT_PLAIN") ? 1.0 : 0.0;
    return v;
}
// the search's parameters for a population of n particles (sharded: the ranks' total)
static inline BisInit bis_init(double beta0, double target_eff, double tol, int64_t n) {
    return {beta0, target_eff, tol, log((double)n), (double)n, bis_plain_mode()};
}

// ---- host side of the state record -----------------------------------------------------------------------------------------
// where the record and k_bis_sums' arrival counter live
static inline void bis_state(asmc_ctx* ctx, double** d_st, unsigned int** d_ticket) {
    *d_st = ctx->d_small + DS_BISECT;
    *d_ticket = reinterpret_cast<unsigned int*>(ctx->d_keys + KEYS_SEARCH_TICKET);  // zeroed by asmc_weights_max_launch
}
// state record S_r (after r closed rounds) of the folded sharded search: two buffers, S_r in buffer r & 1 - the kernel that
// closes round r - 1 reads S_{r-1} while its block 0 writes S_r
static inline double* shard_state_buf(asmc_ctx* ctx, int r) { return ctx->d_small + DS_BISECT + ((r & 1) ? DS_BISECT_REC : 0); }
// the 13-value result of include/asmc.h (asmc_find_beta) from a state record on the host; `n_nan`: the NaN census to report
static inline void bis_result(double* out, const double* h, double n_nan) {
    out[0] = h[BIS_BMIN];      // beta_min = beta*
    out[1] = h[BIS_BMAX];      // beta_max
    out[2] = h[BIS_DONE];      // converged flag
    out[3] = h[BIS_ROUNDS];    // device rounds
    out[4] = h[BIS_EFF_ONE];   // ESS(1.0)/N
    out[5] = n_nan;            // NaN log-weights
    out[6] = h[BIS_TRIP_M];    // (m, S1, S2) of the log-sum-exp at beta*, valid when out[9] != 0
    out[7] = h[BIS_TRIP_S1];
    out[8] = h[BIS_TRIP_S2];
    out[9] = h[BIS_TRIP_OK];
    out[10] = h[BIS_M_ONE];    // (m, S1, S2) at beta = 1
    out[11] = h[BIS_S1_ONE];
    out[12] = h[BIS_S2_ONE];
}
// ---- one round's sums: sixteen equally spaced candidates per particle (k_bis_sums, k_is_weights) -----------------------------
// The grid a round evaluates: c1, c2 and the log-sum-exp shift m1 of the LOWEST candidate, the spacing h and Delta_max
// (BIS_C1 .. BIS_DMAX of the state record).
struct BisGrid {
    double c1, c2, m1, h, dmax;
};
// first round: the leftmost leaf of the four-level tree of [beta0, 1] and sixteenths of the bracket above it, shifted by
// `m_loc` - the maximum at beta = 1 the caller knows (the grid's, the rank's or the block's own)
__device__ __forceinline__ BisGrid bis_first_grid(double beta0, double m_loc) {
    double b1 = 1.0;
    for (int lev = 0; lev < BIS_LEVELS; lev++) b1 = 0.5 * (b1 + beta0);  // leftmost leaf of the first tree
    const double inv = 1.0 / (1.0 - beta0);
    BisGrid g;
    g.c1 = beta0 - b1, g.c2 = b1 - beta0, g.m1 = m_loc * ((b1 - beta0) * inv), g.h = (1.0 - beta0) / 16.0, g.dmax = m_loc * inv;
    return g;
}
// later rounds: the grid the previous round's tail left in the record
__device__ __forceinline__ BisGrid bis_next_grid(const double* st) {
    BisGrid g;
    g.c1 = st[BIS_C1], g.c2 = st[BIS_C2], g.m1 = st[BIS_M1], g.h = st[BIS_H], g.dmax = st[BIS_DMAX];
    return g;
}
// Two particles' terms into the sixteen candidates' S1, S2 (ascending beta): e, e2 = exp(lw(beta_1) - m_1), r, r2 = the ratios of
// their geometric progressions (0, 0 for a particle that is not there).  The order of the additions is the results' bits.
__device__ __forceinline__ void bis_accumulate(double (&s1)[16], double (&s2)[16], double e, double r, double e2, double r2) {
#pragma unroll
    for (int j = 0; j < 16; j++) {
        s1[j] += e;
        s2[j] += e * e;
        e *= r;
        s1[j] += e2;
        s2[j] += e2 * e2;
        e2 *= r2;
    }
}
// The block's partial record records[32 blockIdx.x + 0..31] from every thread's accumulators; s_p: LDS of [waves][32].  Column 2 c + {0: S1, 1: S2},
// c = bis_col_of_sorted(j): heap index of sorted candidate j, 15 = the bracket's upper end.
// Wave level: a butterfly reduce-scatter - at distance o a lane keeps one half of its values and trades the other half with its
// partner, so 16+8+4+2+1+1 = 32 values cross lanes instead of 32 x 6 (the cross-lane permutes run on the LDS pipe, which 8
// waves per CU share; the plain per-value butterflies cost more than the two exponentials per particle); lane l ends up with
// the wave total of column l >> 1.  Then threads 0-31 add the waves' totals in wave order.  The stores are wave 0's.
template <int WAVES>
__device__ __forceinline__ void bis_block_record(const double (&s1)[16], const double (&s2)[16], double (*s_p)[32], double* records) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double vals[32];
#pragma unroll
    for (int j = 0; j < 16; j++) {
        vals[2 * bis_col_of_sorted(j)] = s1[j];
        vals[2 * bis_col_of_sorted(j) + 1] = s2[j];
    }
#pragma unroll
    for (int o = 32, cnt = 32; o >= 2; o >>= 1, cnt >>= 1) {
        const bool up = (lane & o) != 0;
#pragma unroll
        for (int k = 0; k < cnt / 2; k++) {
            const double keep = up ? vals[k + cnt / 2] : vals[k];
            const double send = up ? vals[k] : vals[k + cnt / 2];
            vals[k] = keep + __shfl_xor(send, o, 64);
        }
    }
    vals[0] += __shfl_xor(vals[0], 1, 64);
    if ((lane & 1) == 0) s_p[wave][lane >> 1] = vals[0];
    __syncthreads();
    if (threadIdx.x < 32) {
        double v = s_p[0][threadIdx.x];
        for (int w = 1; w < WAVES; w++) v += s_p[w][threadIdx.x];
        records[(size_t)blockIdx.x * 32 + threadIdx.x] = v;
    }
}

// In-launch hand-off to the block that arrives last (counter form): every block has stored its partial record; the storing
// wave drains its stores, the block meets, ONE lane releases at agent scope and draws a ticket; the block that draws `winning`
// acquires and goes on to read every block's record.  `reset`: the winner zeroes the counter for the next launch (else the counter
// only grows and `winning` moves with it).  Returns, in every thread of the block, whether this block is the last one.
__device__ __forceinline__ bool bis_last_block(unsigned int* ticket, unsigned int winning, bool reset) {
    __shared__ int s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned int t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (t == winning);
        if (s_last) {
            if (reset) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    return s_last != 0;
}

// Closes a search round: fixed-order reduction of the block partials, ESS of every candidate (one lane each), the
// decisions and the sixteen nodes of the next round (asmc_bisect.h: plain 16-ary step or a window around the predicted
// root).  Runs in the LAST block of the round's reduction kernel (k_bis_sums).
//   first round: the 15 heap-ordered midpoints of [beta0, 1] AND beta = 1 itself (16th column; smc/base.py:170-175:
//   eff(1) >= target ends the search at beta* = 1); this round also creates the state record.
//   Stabilising maxima are not searched for: at beta >= beta0 every log-weight is (beta - beta0) * Delta_i up to
//   rounding, so max_i lw_i(beta) = m(1) (beta - beta0)/(1 - beta0) to rounding as well (m(1): exact, from the max
//   kernel), and a log-sum-exp only needs a shift near the maximum, not the maximum itself.
// Fixed-order reduction of the block partial records (32 columns) into s_S; valid after the next __syncthreads().
__device__ __forceinline__ void bis_reduce_partials(const double* __restrict__ partials, int nblocks,
                                                    double (*s_red)[33], double* s_S) {
    const int col = threadIdx.x & 31, part = threadIdx.x >> 5, nparts = blockDim.x >> 5;
    double v = 0.0;
    for (int b0 = part; b0 < nblocks; b0 += 16 * nparts) {  // sixteen records in flight per thread, fixed order
        double t16[16];
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const int b = b0 + q * nparts;
            t16[q] = b < nblocks ? partials[(size_t)b * 32 + col] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 16; q++) v += t16[q];
    }
    s_red[part][col] = v;
    __syncthreads();
    if (threadIdx.x < 32) {
        double t = 0.0;
        for (int q = 0; q < nparts; q++) t += s_red[q][threadIdx.x];
        s_S[threadIdx.x] = t;
    }
}

// The same reduction for records whose sums were shifted by each block's OWN maximum (first round of k_is_weights: no
// grid-wide maximum pass in front of it).  The first round's candidates are beta0 + ks (1 - beta0) / 16, ks = 1 .. 16, so
// record b, candidate ks, power pw in {1, 2} is rescaled to the merged maximum M by
//     exp(lw - m_b t) = exp(lw - M t) exp((m_b - M) / 16)^(pw ks),   t = ks / 16
// (what k_bis_decide does with the ranks' records of a sharded search): ONE exponential per record and an integer power.
// `mrec`: (m_b, NaN count) per block; a block without a finite log-weight (its sums are zero) counts as m_b = M.
// Also returns the merged maximum and the NaN census in s_mn[0], s_mn[1].  nblocks <= 512.
__device__ __forceinline__ void bis_reduce_partials_scaled(const double* __restrict__ partials, const double* __restrict__ mrec,
                                                           int nblocks, double (*s_red)[33], double* s_S, double* s_base,
                                                           double* s_mn) {
    const int col = threadIdx.x & 31, part = threadIdx.x >> 5, nparts = blockDim.x >> 5;
    const int ks = bis_sorted_of_col(col >> 1) + 1;  // sorted position (1 .. 16) of this thread's heap column
    double t16[16];
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const int b = part + q * nparts;
        t16[q] = b < nblocks ? partials[(size_t)b * 32 + col] : 0.0;
    }
    const int b_own = threadIdx.x;  // blockDim.x = 512 >= nblocks
    const double m_own = b_own < nblocks ? mrec[2 * b_own] : -INFINITY, n_own = b_own < nblocks ? mrec[2 * b_own + 1] : 0.0;
    {
        double v = wave_max(m_own == m_own ? m_own : -INFINITY), c = wave_sum(n_own);  // (integer-valued counts: any order)
        if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6][0] = v, s_red[threadIdx.x >> 6][1] = c;
    }
    __syncthreads();
    double m_all = -INFINITY, nan_total = 0.0;
    for (int x = 0; x < (int)(blockDim.x >> 6); x++) m_all = fmax(m_all, s_red[x][0]), nan_total += s_red[x][1];
    if (threadIdx.x == 0) s_mn[0] = m_all, s_mn[1] = nan_total;
    s_base[b_own] = (m_own > -INFINITY && m_all > -INFINITY) ? exp((m_own - m_all) * (1.0 / 16.0)) : 1.0;
    __syncthreads();
    const int e0 = ((col & 1) ? 2 : 1) * ks;  // 1 .. 32
    double v = 0.0;
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const int b = part + q * nparts;
        double f = 1.0, pw = b < nblocks ? s_base[b] : 1.0;
#pragma unroll
        for (int bit = 0; bit < 6; bit++) {
            if ((e0 >> bit) & 1) f *= pw;
            pw *= pw;
        }
        v += t16[q] * f;
    }
    s_red[part][col] = v;
    __syncthreads();
    if (threadIdx.x < 32) {
        double tt = 0.0;
        for (int q = 0; q < nparts; q++) tt += s_red[q][threadIdx.x];
        s_S[threadIdx.x] = tt;
    }
}

// Block-local copy of the search state: the record (BIS_* of asmc_bisect.h) and the candidates' c1, c2, m, shift
// (in: m of this round's candidates; out: those of the next round)
struct BisLds {
    double st[BIS_STATE_LEN];
    double bp[4][16];
};

__device__ __forceinline__ void bis_lds_init(BisLds& L, const BisInit& init, double m_one, double nan_total) {
    if (threadIdx.x < BIS_STATE_LEN) {
        const int i = threadIdx.x;
        L.st[i] = i == BIS_BMIN ? init.beta0 : i == BIS_BMAX ? 1.0 : i == BIS_TARGET ? init.target : i == BIS_TOL ? init.tol
                  : i == BIS_LOGN ? init.logN : i == BIS_BETA0 ? init.beta0 : i == BIS_N ? init.N : i == BIS_M_ONE ? m_one
                  : i == BIS_NAN ? nan_total : i == BIS_MODE ? init.plain : 0.0;
    }
}

// Closes a round on the block-local state.  Precondition: L and s_S are filled and a __syncthreads() lies behind
// that; returns behind a __syncthreads() with L.st[BIS_DONE], L.st[BIS_NEWPACK] (a new candidate grid was chosen) up to date.
// Lanes 0-15: the floats of this round's sixteen nodes (asmc_bisect.h: bis_node_beta - exactly the values the sequential
// loop would hold), their shifts and ESS/N; lane 0: the decisions and the next grid (bis_plan).
__device__ __forceinline__ void bis_tail_core(BisLds& L, bool first, const double* s_S, double* s_eff) {
    double(&s_st)[BIS_STATE_LEN] = L.st;
    if (threadIdx.x < 16) {
        const int j = threadIdx.x;
        const double beta0 = s_st[BIS_BETA0], m_one = s_st[BIS_M_ONE];
        const int LU = first ? 4 : (int)s_st[BIS_LU];
        const long long K = first ? (long long)(j + 1) : (long long)s_st[BIS_KFIRST] + j * (long long)s_st[BIS_STRIDE];
        const double b = bis_node_beta(K, LU, beta0);
        const double mj = m_one * ((b - beta0) * (1.0 / (1.0 - beta0)));
        const int c = bis_col_of_sorted(j);
        const double e = ess_over_n(mj, s_S[2 * c], s_S[2 * c + 1], s_st[BIS_LOGN], s_st[BIS_N]);
        L.bp[0][j] = b;
        L.bp[1][j] = log(e) - log(s_st[BIS_TARGET]);
        L.bp[2][j] = mj;
        s_eff[j] = e;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double r[BIS_STATE_LEN];  // the record in registers: the decision chain pays no LDS round trip per access
#pragma unroll
        for (int i = 0; i < BIS_STATE_LEN; i++) r[i] = s_st[i];
        bis_plan(r, first, L.bp[0], L.bp[2], s_eff, L.bp[1], s_S);
#pragma unroll
        for (int i = 0; i < BIS_STATE_LEN; i++) s_st[i] = r[i];
    }
    __syncthreads();
}

// Round tail on the state record in global memory (one launch per round: k_bis_sums' last block, k_bis_decide).
// `partials` == nullptr: s_S already holds the column sums (sharded search: the rank records merged by k_bis_decide).
__device__ __forceinline__ void bis_tail_body(double* __restrict__ st, const double* __restrict__ partials, int nblocks,
                                              bool first, double m_one_in, const BisInit& init, double (*s_red)[33],
                                              double* s_S, double* s_eff, double nan_total = 0.0) {
    // the state record is staged in LDS: lane 0's decision chain must not pay a global-memory latency per dependent access
    __shared__ BisLds L;
    if (first)
        bis_lds_init(L, init, m_one_in, nan_total);
    else if (threadIdx.x < BIS_STATE_LEN)
        L.st[threadIdx.x] = st[threadIdx.x];
    if (partials) bis_reduce_partials(partials, nblocks, s_red, s_S);
    __syncthreads();
    bis_tail_core(L, first, s_S, s_eff);
    if (threadIdx.x < BIS_STATE_LEN) st[threadIdx.x] = L.st[threadIdx.x];
}

// heap node k of the bisection tree rooted at (lo, hi): the midpoint the sequential loop would try there
__device__ __forceinline__ double bis_heap_mid(int k, double lo, double hi) {
    const int kp = k + 1;
    const int depth = 31 - __clz(kp);
    double mid = 0.5 * (hi + lo);
    for (int lev = depth - 1; lev >= 0; lev--) {
        if ((kp >> lev) & 1)
            lo = mid;  // right child: eff >= target there
        else
            hi = mid;
        mid = 0.5 * (hi + lo);
    }
    return mid;
}

// The ranks' records of round `round` of a sharded search (recs[world][ASMC_BIS_REC]: 32 column sums, the shift base they are
// relative to, the rank's NaN census) merged in rank order into s_S[0..31] (threads 0-31; valid behind the next __syncthreads()).
// First round: the ranks reduced against their LOCAL m(1); the sums are rescaled to the merged maximum M = max_r m_r(1),
// exp(lw - m_r t) = exp(lw - M t) exp((M - m_r) t) with t = (beta - beta0)/(1 - beta0).  Later rounds use M on every rank.
// Returns M; nan_total: the merged census (first round; 0 later).
__device__ __forceinline__ double bis_merge_records(const double* __restrict__ recs, int world, int round, double beta0,
                                                    double* s_S, double& nan_total) {
    double m_all = recs[32];
    nan_total = 0.0;
    for (int r = 1; r < world; r++) m_all = fmax(m_all, recs[(size_t)r * ASMC_BIS_REC + 32]);
    if (round == 0)
        for (int r = 0; r < world; r++) nan_total += recs[(size_t)r * ASMC_BIS_REC + 33];
    if (threadIdx.x < 32) {
        const int c = threadIdx.x, k = c >> 1;
        double acc = 0.0;
        if (round == 0) {
            const double beta = k < BIS_NODES ? bis_heap_mid(k, beta0, 1.0) : 1.0;
            const double t = (beta - beta0) * (1.0 / (1.0 - beta0));
            const double pw = (c & 1) ? 2.0 : 1.0;
            for (int r = 0; r < world; r++) {
                const double mr = recs[(size_t)r * ASMC_BIS_REC + 32];
                acc += recs[(size_t)r * ASMC_BIS_REC + c] * exp(pw * (mr * t - m_all * t));
            }
        } else {
            for (int r = 0; r < world; r++) acc += recs[(size_t)r * ASMC_BIS_REC + c];
        }
        s_S[c] = acc;
    }
    return m_all;
}

// Sharded search, the decide half of round `round` on a BLOCK-LOCAL state (what k_bis_decide does on the record in global
// memory): merges the ranks' records in rank order and closes the round.  Every block of the NEXT kernel of the chain runs
// it redundantly from the same gathered records (fixed order: the same bits everywhere), so the round costs no launch of its
// own.  `st_prev`: the state record after the previous round (unused in round 0, which creates it).  Returns behind a
// __syncthreads(); a search that had converged earlier passes through unchanged.
__device__ __forceinline__ void bis_shard_decide(BisLds& L, const double* __restrict__ recs, int world, int round,
                                                 const BisInit& init, const double* __restrict__ st_prev, double* s_S,
                                                 double* s_eff) {
    if (round > 0) {
        if (threadIdx.x < BIS_STATE_LEN) L.st[threadIdx.x] = st_prev[threadIdx.x];
        __syncthreads();
        if (L.st[BIS_DONE] != 0.0) return;  // converged earlier (uniform: every thread reads the same value)
    }
    double nan_total;
    const double m_all = bis_merge_records(recs, world, round, init.beta0, s_S, nan_total);
    if (round == 0) bis_lds_init(L, init, m_all, nan_total);
    __syncthreads();
    bis_tail_core(L, round == 0, s_S, s_eff);
}

