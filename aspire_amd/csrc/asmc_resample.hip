// asmc_resample.hip — PCG64 uniforms, upper-bound search, row gather, validity compaction, ordered range selection,
// the fused importance step.  (The cdf scans the search reads are asmc_cdf.hip.)
//
// Replaces (reference mj-will/aspire):
//   src/aspire/samples.py:1277-1278  w = exp(lw - LSE); idx = rng.choice(N, n, True, p=w)
//     == numpy Generator.choice: cdf = cumsum(w); cdf /= (its last entry); u = random(n);
//        idx = cdf.searchsorted(u, side="right")                      
//   src/aspire/samples.py:1279-1287  x[idx], log_likelihood[idx], log_prior[idx], log_q[idx]
//   src/aspire/samplers/mcmc.py:88-108  finite-mask filter of draw_initial_samples
//
#include <stdlib.h>

#include "asmc_common.h"

// ---- ordered range selection: out = u[(lo <= u) & (u < hi)] in index order (count / scan / scatter) ------------------
__global__ __launch_bounds__(ASMC_BLOCK) void k_range_count(int64_t n, const double* __restrict__ u,
                                                           const double* __restrict__ lohi,
                                                           long long* __restrict__ tiles) {
    const double lo = lohi[0], hi = lohi[1];
    const int64_t base = (int64_t)blockIdx.x * ASMC_SCAN_TILE + (int64_t)threadIdx.x * (ASMC_SCAN_TILE / ASMC_BLOCK);
    long long c = 0;
#pragma unroll
    for (int j = 0; j < ASMC_SCAN_TILE / ASMC_BLOCK; j++)
        if (base + j < n) {
            const double v = u[base + j];
            c += (v >= lo && v < hi) ? 1 : 0;
        }
    __shared__ long long s_p[ASMC_BLOCK / 64];
    c = wave_sum_ll(c);
    if ((threadIdx.x & 63) == 0) s_p[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tiles[blockIdx.x] = s_p[0] + s_p[1] + s_p[2] + s_p[3];
}

// =============================================================================================
// PCG64 (XSL-RR 128/64) uniforms — numpy.random.PCG64 stream, parallel through LCG jump-ahead
// =============================================================================================
struct U128 {
    unsigned long long lo, hi;
};
__host__ __device__ __forceinline__ U128 u128_mul(U128 a, U128 b) {
    U128 r;
    r.lo = a.lo * b.lo;
#if defined(__HIP_DEVICE_COMPILE__)
    r.hi = __umul64hi(a.lo, b.lo) + a.lo * b.hi + a.hi * b.lo;
#else
    r.hi = (unsigned long long)(((unsigned __int128)a.lo * b.lo) >> 64) + a.lo * b.hi + a.hi * b.lo;
#endif
    return r;
}
__host__ __device__ __forceinline__ U128 u128_add(U128 a, U128 b) {
    U128 r;
    r.lo = a.lo + b.lo;
    r.hi = a.hi + b.hi + (r.lo < a.lo ? 1ULL : 0ULL);
    return r;
}

#define PCG_THREADS_LOG2 16
#define PCG_THREADS (1 << PCG_THREADS_LOG2)

// tab[i] = {A_lo, A_hi, C_lo, C_hi} for a jump of 2^i steps
__global__ __launch_bounds__(ASMC_BLOCK) void k_pcg64_uniforms(const unsigned long long* __restrict__ tab,
                                                              U128 state0, unsigned long long offset,
                                                              int64_t n, double* __restrict__ u) {
    const unsigned long long j = (unsigned long long)blockIdx.x * ASMC_BLOCK + threadIdx.x;
    if ((int64_t)j >= n) return;
    // post-step state of draw j: advance(state0, offset + j + 1)
    unsigned long long delta = offset + j + 1ULL;
    U128 st = state0;
    for (int b = 0; b < 64 && delta; b++, delta >>= 1) {
        if (delta & 1ULL) {
            U128 A = {tab[4 * b], tab[4 * b + 1]}, C = {tab[4 * b + 2], tab[4 * b + 3]};
            st = u128_add(u128_mul(st, A), C);
        }
    }
    const U128 AT = {tab[4 * PCG_THREADS_LOG2], tab[4 * PCG_THREADS_LOG2 + 1]};
    const U128 CT = {tab[4 * PCG_THREADS_LOG2 + 2], tab[4 * PCG_THREADS_LOG2 + 3]};
    for (int64_t i = (int64_t)j; i < n; i += PCG_THREADS) {
        const unsigned long long x = st.hi ^ st.lo;
        const unsigned rot = (unsigned)(st.hi >> 58);
        const unsigned long long out = (x >> rot) | (x << ((64u - rot) & 63u));
        u[i] = (double)(out >> 11) * (1.0 / 9007199254740992.0);
        st = u128_add(u128_mul(st, AT), CT);
    }
}

// Sharded owner-layout resampling: all n_total draws of the stream are generated on every rank; a wave keeps those
// inside this rank's cdf slice [lo, hi) in its own segment of `stage` (no atomics: the order of the kept draws is
// (wave, iteration, lane), a fixed function of the draw index), mapped to the local cdf's coordinate.
#define SEL_LOG2 18  // log2(ASMC_SELECT_THREADS): 4096 waves keep every SIMD busy (65536 threads: 17 us per 2M draws)
#define SEL_WAVES (ASMC_SELECT_THREADS / 64)
__global__ __launch_bounds__(ASMC_BLOCK) void k_pcg64_select(const unsigned long long* __restrict__ tab, U128 state0,
                                                            int64_t n, double lo, double hi, int64_t iters,
                                                            double* __restrict__ stage,
                                                            long long* __restrict__ counts) {
    const unsigned long long j = (unsigned long long)blockIdx.x * ASMC_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)(j >> 6);
    unsigned long long delta = j + 1ULL;
    U128 st = state0;
    for (int b = 0; b < 64 && delta; b++, delta >>= 1) {
        if (delta & 1ULL) {
            U128 A = {tab[4 * b], tab[4 * b + 1]}, C = {tab[4 * b + 2], tab[4 * b + 3]};
            st = u128_add(u128_mul(st, A), C);
        }
    }
    const U128 AT = {tab[4 * SEL_LOG2], tab[4 * SEL_LOG2 + 1]};
    const U128 CT = {tab[4 * SEL_LOG2 + 2], tab[4 * SEL_LOG2 + 3]};
    const double inv_w = 1.0 / (hi - lo);
    double* seg = stage + wave * 64 * iters;
    long long pos = 0;
    for (int64_t k = 0; k < iters; k++) {
        const int64_t i = k * ASMC_SELECT_THREADS + (int64_t)j;
        const unsigned long long x = st.hi ^ st.lo;
        const unsigned rot = (unsigned)(st.hi >> 58);
        const unsigned long long out = (x >> rot) | (x << ((64u - rot) & 63u));
        const double u = (double)(out >> 11) * (1.0 / 9007199254740992.0);
        const bool keep = i < n && u >= lo && u < hi;
        const unsigned long long mask = __ballot(keep);
        if (keep) {
            double q = (u - lo) * inv_w;
            if (q >= 1.0) q = 0x1.fffffffffffffp-1;
            seg[pos + __popcll(mask & ((1ULL << lane) - 1ULL))] = q;
        }
        pos += __popcll(mask);
        st = u128_add(u128_mul(st, AT), CT);
    }
    if (lane == 0) counts[wave] = pos;
}

// exclusive scan of the SEL_WAVES wave counts; offsets behind the counts, the total behind the offsets
__global__ __launch_bounds__(1024) void k_select_scan(long long* __restrict__ counts) {
    constexpr int PER = SEL_WAVES / 1024;  // consecutive counts per thread
    __shared__ long long s[1024];
    const int t = threadIdx.x;
    long long loc[PER], tot = 0;
#pragma unroll
    for (int q = 0; q < PER; q++) {
        loc[q] = counts[t * PER + q];
        tot += loc[q];
    }
    s[t] = tot;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const long long v = t >= o ? s[t - o] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    long long run = s[t] - tot;  // exclusive prefix of this thread's first count
#pragma unroll
    for (int q = 0; q < PER; q++) {
        counts[SEL_WAVES + t * PER + q] = run;
        run += loc[q];
    }
    if (t == 1023) counts[2 * SEL_WAVES] = s[t];
}

__global__ __launch_bounds__(64) void k_select_compact(int64_t iters, const double* __restrict__ stage,
                                                       const long long* __restrict__ counts,
                                                       double* __restrict__ q) {
    const int64_t wave = blockIdx.x;
    const long long cnt = counts[wave], off = counts[SEL_WAVES + wave];
    const double* seg = stage + wave * 64 * iters;
    for (long long t = threadIdx.x; t < cnt; t += 64) q[off + t] = seg[t];
}

__global__ __launch_bounds__(ASMC_BLOCK) void k_systematic(int64_t n_out, int64_t j0, int64_t n_total,
                                                          double u0, const double* __restrict__ v,
                                                          double* __restrict__ u) {
    const int64_t stride = (int64_t)gridDim.x * ASMC_BLOCK;
    for (int64_t j = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x; j < n_out; j += stride) {
        const double off = v ? v[j] : u0;
        u[j] = ((double)(j0 + j) + off) / (double)n_total;
    }
}

// =============================================================================================
// search: idx[j] = #{k : cdf[k] <= u[j]}   (searchsorted side="right")
// =============================================================================================
__global__ __launch_bounds__(ASMC_BLOCK) void k_search(int64_t n, const double* __restrict__ cdf,
                                                      int64_t n_out, const double* __restrict__ u,
                                                      int64_t* __restrict__ idx) {
    const int64_t stride = (int64_t)gridDim.x * ASMC_BLOCK;
    for (int64_t j = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x; j < n_out; j += stride) {
        const double key = u[j];
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (cdf[mid] <= key)
                lo = mid + 1;
            else
                hi = mid;
        }
        // a key below 1 names a row: a cdf whose last element fell below the key (an unnormalised one, a rounding) must not
        // send n to the gather (k_search_pcg's clamp).  Keys >= 1 keep numpy's answer n; a NaN key gives 0 (no cdf[k] <= NaN)
        idx[j] = (lo >= n && key < 1.0) ? n - 1 : lo;
    }
}

// Guided search.  A guide table G[b] = #{k : cdf[k] <= b / NB}, b = 0..NB, is built from NB + 1 binary searches with
// SORTED queries (neighbouring threads walk the same cache lines, so the build is cheap), and every lookup then
// only searches the window [G[b], G[b+1]] of its bucket b = floor(u NB): about two random cache lines per output
// instead of the ~6 cold levels of a full binary search over the 8 MB cdf.  The result is the same upper bound.
__global__ __launch_bounds__(ASMC_BLOCK) void k_guide_build(int64_t n, const double* __restrict__ cdf, int64_t nb,
                                                           unsigned int* __restrict__ guide) {
    const int64_t stride = (int64_t)gridDim.x * ASMC_BLOCK;
    for (int64_t b = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x; b <= nb; b += stride) {
        const double key = (double)b / (double)nb;
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (cdf[mid] <= key)
                lo = mid + 1;
            else
                hi = mid;
        }
        guide[b] = (unsigned int)lo;
    }
}

__global__ __launch_bounds__(ASMC_BLOCK) void k_search_guided(int64_t n, const double* __restrict__ cdf, int64_t nb,
                                                             const unsigned int* __restrict__ guide, int64_t n_out,
                                                             const double* __restrict__ u, int64_t* __restrict__ idx) {
    const int64_t stride = (int64_t)gridDim.x * ASMC_BLOCK;
    const double fnb = (double)nb;
    for (int64_t j = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x; j < n_out; j += stride) {
        const double key = u[j];
        int64_t lo = 0, hi = n;
        if (key >= 0.0 && key < 1.0) {
            int64_t b = (int64_t)(key * fnb);
            b = b > nb - 1 ? nb - 1 : b;
            // make b / NB <= key < (b + 1) / NB hold for the very expressions the table was built with
            while (b > 0 && (double)b / fnb > key) b--;
            while (b < nb - 1 && (double)(b + 1) / fnb <= key) b++;
            lo = guide[b];
            hi = guide[b + 1];
        }
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (cdf[mid] <= key)
                lo = mid + 1;
            else
                hi = mid;
        }
        // (the clamp of k_search, for the same reason)
        idx[j] = (lo >= n && key < 1.0) ? n - 1 : lo;
    }
}

// k_pcg64_uniforms + k_search_guided in one pass (asmc_importance_step): 2^SP_LOG2 threads, thread j takes the draws
// j, j + T, j + 2T, ... of the stream (one jump-ahead per thread, then strides of T), four at a time so that four
// independent lookups are in flight per lane; the uniforms never touch memory.
#define SP_LOG2 18
__global__ __launch_bounds__(ASMC_BLOCK) void k_search_pcg(const unsigned long long* __restrict__ tab, U128 state0,
                                                          int tlog2, int64_t n, const double* __restrict__ cdf,
                                                          int64_t nb, const unsigned int* __restrict__ guide,
                                                          int64_t n_out, int64_t* __restrict__ idx) {
    const int64_t T = (int64_t)1 << tlog2;
    const unsigned long long j = (unsigned long long)blockIdx.x * ASMC_BLOCK + threadIdx.x;
    if ((int64_t)j >= T || (int64_t)j >= n_out) return;
    unsigned long long delta = j + 1ULL;  // post-step state of draw j: advance(state0, j + 1)
    U128 st = state0;
    for (int b = 0; b < 64 && delta; b++, delta >>= 1) {
        if (delta & 1ULL) {
            U128 A = {tab[4 * b], tab[4 * b + 1]}, C = {tab[4 * b + 2], tab[4 * b + 3]};
            st = u128_add(u128_mul(st, A), C);
        }
    }
    const U128 AT = {tab[4 * tlog2], tab[4 * tlog2 + 1]};
    const U128 CT = {tab[4 * tlog2 + 2], tab[4 * tlog2 + 3]};
    const double fnb = (double)nb;
    for (int64_t i0 = (int64_t)j; i0 < n_out; i0 += 4 * T) {
        double key[4];
        int64_t lo[4], hi[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            lo[q] = 0, hi[q] = 0, key[q] = 0.0;
            if (i0 + q * T < n_out) {
                const unsigned long long x = st.hi ^ st.lo;
                const unsigned rot = (unsigned)(st.hi >> 58);
                const unsigned long long out = (x >> rot) | (x << ((64u - rot) & 63u));
                key[q] = (double)(out >> 11) * (1.0 / 9007199254740992.0);
                st = u128_add(u128_mul(st, AT), CT);
                hi[q] = n;
                if (guide) {
                    int64_t b = (int64_t)(key[q] * fnb);
                    b = b > nb - 1 ? nb - 1 : b;
                    // make b / NB <= key < (b + 1) / NB hold for the very expressions the table was built with
                    while (b > 0 && (double)b / fnb > key[q]) b--;
                    while (b < nb - 1 && (double)(b + 1) / fnb <= key[q]) b++;
                    lo[q] = guide[b];
                    hi[q] = guide[b + 1];
                }
            }
        }
        bool any = true;
        while (any) {
            any = false;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if (lo[q] < hi[q]) {
                    const int64_t mid = lo[q] + ((hi[q] - lo[q]) >> 1);
                    if (cdf[mid] <= key[q])
                        lo[q] = mid + 1;
                    else
                        hi[q] = mid;
                }
                any |= lo[q] < hi[q];
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (i0 + q * T < n_out) idx[i0 + q * T] = lo[q] < n ? lo[q] : n - 1;  // (== lo: u < 1 = cdf[n-1]; a garbage cdf must not index past the rows)
    }
}

// =============================================================================================
// gather rows
// =============================================================================================
// 16-byte chunks: chunk c -> (row = c / cpr, col = c % cpr); lanes of a wave cover whole rows, so
// every random row is fetched as full 64-B+ bursts and the output is written fully coalesced.
// power-of-two rows (cpr = 2^SH 16-byte chunks): shifts instead of 64-bit divisions, four chunks in flight per lane,
// non-temporal stores (the output is not re-read by this kernel and should not displace the cdf / input rows in L2)
// The three log-probabilities of the gathered rows: one output per lane, coalesced stores.  A random 8-byte read costs
// a whole sector request, and at 1M x 32 fp64 the three of them per draw cost 40 % of the gather; with `rec` (the
// source's (ll, lp, lq, 0) records, k_pack_records) a draw reads one 32-byte sector instead.
struct alignas(32) LogRec {
    double ll, lp, lq, pad;
};
__global__ __launch_bounds__(ASMC_BLOCK) void k_pack_records(int64_t n, const double* __restrict__ ll, const double* __restrict__ lp,
                                                            const double* __restrict__ lq, LogRec* __restrict__ rec) {
    const int64_t stride = (int64_t)gridDim.x * ASMC_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x; i < n; i += stride) rec[i] = LogRec{ll[i], lp[i], lq[i], 0.0};
}
__device__ __forceinline__ void gather_scalars(int64_t n_out, const int64_t* __restrict__ idx, const LogRec* __restrict__ rec,
                                               const double* __restrict__ ll_in, const double* __restrict__ lp_in,
                                               const double* __restrict__ lq_in, double* __restrict__ ll_out,
                                               double* __restrict__ lp_out, double* __restrict__ lq_out) {
    const int64_t stride = (int64_t)gridDim.x * ASMC_BLOCK;
    for (int64_t j = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x; j < n_out; j += stride) {
        const int64_t s = idx[j];
        double a, b, c;
        if (rec) {
            const LogRec r = rec[s];
            a = r.ll, b = r.lp, c = r.lq;
        } else {
            a = ll_in[s], b = lp_in[s], c = lq_in[s];
        }
        __builtin_nontemporal_store(a, &ll_out[j]);
        __builtin_nontemporal_store(b, &lp_out[j]);
        __builtin_nontemporal_store(c, &lq_out[j]);
    }
}

// CS: the rows are fp64 - the column sums of the gathered rows ride along (a lane always handles the same 16-byte piece of a
// row: the grid stride is a multiple of the pieces per row), one partial row of d sums per block in cs_partials; the
// reference fit behind the gather (asmc_mean_gram_enqueue) then needs no column-sum pass over the rows (70 us at 1M x 32).
template <int SH, bool CS>
__global__ __launch_bounds__(ASMC_BLOCK) void k_gather16_pow2(int64_t n_out, const int64_t* __restrict__ idx,
                                                             const LogRec* __restrict__ rec,
                                                             const uint4* __restrict__ x_in, uint4* __restrict__ x_out,
                                                             const double* __restrict__ ll_in,
                                                             const double* __restrict__ lp_in,
                                                             const double* __restrict__ lq_in,
                                                             double* __restrict__ ll_out, double* __restrict__ lp_out,
                                                             double* __restrict__ lq_out, double* __restrict__ cs_partials) {
    double cs0 = 0.0, cs1 = 0.0;
#ifdef GATHER_U
    constexpr int U = GATHER_U;
#else
    constexpr int U = 4;
#endif
    const int64_t total = n_out << SH;
    const int64_t stride = (int64_t)gridDim.x * ASMC_BLOCK;
    for (int64_t c0 = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x; c0 < total; c0 += U * stride) {
        int64_t src[U];
        uint4 v[U];
#pragma unroll
        for (int q = 0; q < U; q++) {
            const int64_t c = c0 + q * stride;
            src[q] = c < total ? idx[c >> SH] : 0;
        }
#pragma unroll
        for (int q = 0; q < U; q++) {
            const int64_t c = c0 + q * stride;
            if (c < total) {
#ifdef GATHER_NTLOAD
                const uint4* sp4 = &x_in[(src[q] << SH) + (c & ((1 << SH) - 1))];
                v[q].x = __builtin_nontemporal_load(&sp4->x), v[q].y = __builtin_nontemporal_load(&sp4->y);
                v[q].z = __builtin_nontemporal_load(&sp4->z), v[q].w = __builtin_nontemporal_load(&sp4->w);
#else
                v[q] = x_in[(src[q] << SH) + (c & ((1 << SH) - 1))];
#endif
            }
        }
#pragma unroll
        for (int q = 0; q < U; q++) {
            const int64_t c = c0 + q * stride;
            if (c < total) {
                __builtin_nontemporal_store(v[q].x, &x_out[c].x);
                __builtin_nontemporal_store(v[q].y, &x_out[c].y);
                __builtin_nontemporal_store(v[q].z, &x_out[c].z);
                __builtin_nontemporal_store(v[q].w, &x_out[c].w);
                if (CS) {
                    cs0 += __longlong_as_double((long long)(((unsigned long long)v[q].y << 32) | v[q].x));
                    cs1 += __longlong_as_double((long long)(((unsigned long long)v[q].w << 32) | v[q].z));
                }
            }
        }
    }
    if (CS) {
        constexpr int CPR = 1 << SH;
        __shared__ double s_cs[ASMC_BLOCK / 64][2 * CPR];
#pragma unroll
        for (int o = CPR; o < 64; o <<= 1) {
            cs0 += __shfl_xor(cs0, o, 64);
            cs1 += __shfl_xor(cs1, o, 64);
        }
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane < CPR) s_cs[wave][2 * lane] = cs0, s_cs[wave][2 * lane + 1] = cs1;
        __syncthreads();
        if (threadIdx.x < 2 * CPR) {
            double t = 0.0;
            for (int w = 0; w < ASMC_BLOCK / 64; w++) t += s_cs[w][threadIdx.x];
            cs_partials[(size_t)blockIdx.x * (2 * CPR) + threadIdx.x] = t;
        }
    }
    gather_scalars(n_out, idx, rec, ll_in, lp_in, lq_in, ll_out, lp_out, lq_out);
}

__global__ __launch_bounds__(ASMC_BLOCK) void k_gather16(int64_t n_out, const int64_t* __restrict__ idx,
                                                        const LogRec* __restrict__ rec, int cpr,
                                                        const uint4* __restrict__ x_in,
                                                        uint4* __restrict__ x_out,
                                                        const double* __restrict__ ll_in,
                                                        const double* __restrict__ lp_in,
                                                        const double* __restrict__ lq_in,
                                                        double* __restrict__ ll_out,
                                                        double* __restrict__ lp_out,
                                                        double* __restrict__ lq_out) {
    const int64_t total = n_out * cpr;
    const int64_t stride = (int64_t)gridDim.x * ASMC_BLOCK;
    int64_t c = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x;
    // two chunks in flight per lane
    for (; c + stride < total; c += 2 * stride) {
        const int64_t c1 = c + stride;
        const int64_t r0 = c / cpr, r1 = c1 / cpr;
        const int k0 = (int)(c - r0 * cpr), k1 = (int)(c1 - r1 * cpr);
        const int64_t s0 = idx[r0], s1 = idx[r1];
        const uint4 v0 = x_in[s0 * cpr + k0];
        const uint4 v1 = x_in[s1 * cpr + k1];
        x_out[c] = v0;
        x_out[c1] = v1;
    }
    for (; c < total; c += stride) {
        const int64_t r0 = c / cpr;
        const int k0 = (int)(c - r0 * cpr);
        const int64_t s0 = idx[r0];
        x_out[c] = x_in[s0 * cpr + k0];
    }
    gather_scalars(n_out, idx, rec, ll_in, lp_in, lq_in, ll_out, lp_out, lq_out);
}

// generic element-wise fallback (row bytes not a multiple of 16)
template <typename T>
__global__ __launch_bounds__(ASMC_BLOCK) void k_gather_elem(int64_t n_out, const int64_t* __restrict__ idx,
                                                           const LogRec* __restrict__ rec, int d,
                                                           const T* __restrict__ x_in,
                                                           T* __restrict__ x_out,
                                                           const double* __restrict__ ll_in,
                                                           const double* __restrict__ lp_in,
                                                           const double* __restrict__ lq_in,
                                                           double* __restrict__ ll_out,
                                                           double* __restrict__ lp_out,
                                                           double* __restrict__ lq_out) {
    const int64_t total = n_out * d;
    const int64_t stride = (int64_t)gridDim.x * ASMC_BLOCK;
    for (int64_t c = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x; c < total; c += stride) {
        const int64_t r = c / d;
        const int k = (int)(c - r * d);
        const int64_t s = idx[r];
        x_out[c] = x_in[s * d + k];
    }
    gather_scalars(n_out, idx, rec, ll_in, lp_in, lq_in, ll_out, lp_out, lq_out);
}

// =============================================================================================
// validity compaction (finite log_prior & log_likelihood), order preserving
// =============================================================================================
__device__ __forceinline__ bool row_valid(double ll, double lp) { return isfinite(ll) && isfinite(lp); }

__global__ __launch_bounds__(ASMC_BLOCK) void k_valid_count(int64_t n, const double* __restrict__ ll,
                                                           const double* __restrict__ lp,
                                                           long long* __restrict__ tiles) {
    const int64_t base = (int64_t)blockIdx.x * ASMC_SCAN_TILE + (int64_t)threadIdx.x * SC_E;
    long long c = 0;
#pragma unroll
    for (int j = 0; j < SC_E; j++)
        if (base + j < n && row_valid(ll[base + j], lp[base + j])) c++;
    __shared__ long long s_p[ASMC_BLOCK / 64];
    c = wave_sum_ll(c);
    if ((threadIdx.x & 63) == 0) s_p[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tiles[blockIdx.x] = s_p[0] + s_p[1] + s_p[2] + s_p[3];
}

__global__ __launch_bounds__(64) void k_scan_tiles_ll(int64_t n_tiles, long long* __restrict__ tiles,
                                                     long long* __restrict__ total_out) {
    // single wave, sequential chunks of 64 (n_tiles is small)
    long long carry = 0;
    const int lane = threadIdx.x;
    for (int64_t start = 0; start < n_tiles; start += 64) {
        const int64_t i = start + lane;
        long long v = i < n_tiles ? tiles[i] : 0;
        long long inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            long long t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (i < n_tiles) tiles[i] = carry + inc - v;
        carry += __shfl(inc, 63, 64);
    }
    if (lane == 0) *total_out = carry;
}

template <typename T>
__global__ __launch_bounds__(ASMC_BLOCK) void k_compact_scatter(
    int64_t n, int d, const T* __restrict__ x, const double* __restrict__ ll, const double* __restrict__ lp,
    const double* __restrict__ lq, const long long* __restrict__ tiles, T* __restrict__ x_out,
    double* __restrict__ ll_out, double* __restrict__ lp_out, double* __restrict__ lq_out) {
    const int64_t base = (int64_t)blockIdx.x * ASMC_SCAN_TILE + (int64_t)threadIdx.x * SC_E;
    bool ok[SC_E];
    long long c = 0;
#pragma unroll
    for (int j = 0; j < SC_E; j++) {
        ok[j] = (base + j < n) && row_valid(ll[base + j], lp[base + j]);
        c += ok[j] ? 1 : 0;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        long long t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __shared__ long long s_wave[ASMC_BLOCK / 64];
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    long long dst = tiles[blockIdx.x] + (inc - c);
    for (int k = 0; k < wave; k++) dst += s_wave[k];
#pragma unroll
    for (int j = 0; j < SC_E; j++) {
        if (ok[j]) {
            const int64_t src = base + j;
            for (int k = 0; k < d; k++) x_out[dst * d + k] = x[src * d + k];
            ll_out[dst] = ll[src];
            lp_out[dst] = lp[src];
            lq_out[dst] = lq[src];
            dst++;
        }
    }
}


// k_shard_edges + k_range_count in one launch (the sharded step's chain of launches): every block forms the slice's edges
// itself, with k_shard_edges' own division, and block 0 leaves them in edges_out[4]
__global__ __launch_bounds__(ASMC_BLOCK) void k_range_count_shard(int64_t n, const double* __restrict__ u,
                                                                 const double* __restrict__ state,
                                                                 const double* __restrict__ s_in,
                                                                 const double* __restrict__ cdf_last,
                                                                 long long* __restrict__ tiles,
                                                                 double* __restrict__ edges_out) {
    const double lo = *s_in / state[1], hi = *cdf_last;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        edges_out[0] = state[2] != 0.0 ? 0.0 : 1.0;
        edges_out[1] = state[1];
        edges_out[2] = lo;
        edges_out[3] = hi;
    }
    const int64_t base = (int64_t)blockIdx.x * ASMC_SCAN_TILE + (int64_t)threadIdx.x * (ASMC_SCAN_TILE / ASMC_BLOCK);
    long long c = 0;
#pragma unroll
    for (int j = 0; j < ASMC_SCAN_TILE / ASMC_BLOCK; j++)
        if (base + j < n) {
            const double v = u[base + j];
            c += (v >= lo && v < hi) ? 1 : 0;
        }
    __shared__ long long s_p[ASMC_BLOCK / 64];
    c = wave_sum_ll(c);
    if ((threadIdx.x & 63) == 0) s_p[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tiles[blockIdx.x] = s_p[0] + s_p[1] + s_p[2] + s_p[3];
}

// SELF_SCAN: `tiles` holds the tiles' COUNTS (k_range_count's output as it is) and a block adds up the counts in front of its
// tile itself (integers: any order); the last block leaves info_out = {kept, failure flag of the slice (edges[0])} - the
// k_scan_tiles_ll and k_range_info launches of the step-by-step form
template <bool SELF_SCAN>
__global__ __launch_bounds__(ASMC_BLOCK) void k_range_scatter(int64_t n, const double* __restrict__ u,
                                                             const double* __restrict__ lohi,
                                                             const long long* __restrict__ tiles,
                                                             double* __restrict__ out, long long* __restrict__ info_out) {
    const double lo = lohi[0], hi = lohi[1];
    __shared__ long long s_front;
    if (SELF_SCAN) {
        long long f = 0;
        for (int64_t k = threadIdx.x; k < (int64_t)blockIdx.x; k += ASMC_BLOCK) f += tiles[k];
        f = wave_sum_ll(f);
        __shared__ long long s_f[ASMC_BLOCK / 64];
        if ((threadIdx.x & 63) == 0) s_f[threadIdx.x >> 6] = f;
        __syncthreads();
        if (threadIdx.x == 0) {
            long long tot = 0;
            for (int k = 0; k < ASMC_BLOCK / 64; k++) tot += s_f[k];
            s_front = tot;
            if (blockIdx.x == gridDim.x - 1) {
                info_out[0] = tot + tiles[blockIdx.x];
                info_out[1] = (long long)llrint(lohi[-2]);  // edges[0]
            }
        }
        __syncthreads();
    }
    const int64_t base = (int64_t)blockIdx.x * ASMC_SCAN_TILE + (int64_t)threadIdx.x * SC_E;
    double v[SC_E];
    bool ok[SC_E];
    long long c = 0;
#pragma unroll
    for (int j = 0; j < SC_E; j++) {
        v[j] = (base + j < n) ? u[base + j] : -1.0;
        ok[j] = (base + j < n) && v[j] >= lo && v[j] < hi;
        c += ok[j] ? 1 : 0;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        long long t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __shared__ long long s_wave[ASMC_BLOCK / 64];
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    long long dst = (SELF_SCAN ? s_front : tiles[blockIdx.x]) + (inc - c);
    for (int k = 0; k < wave; k++) dst += s_wave[k];
#pragma unroll
    for (int j = 0; j < SC_E; j++)
        if (ok[j]) out[dst++] = v[j];
}

// =============================================================================================
// host entry points
// =============================================================================================
// one int64 on the device -> *out_host through the front of the pinned staging; waits for the stream
static int read_back_count(asmc_ctx* ctx, const long long* d_count, int64_t* out_host, hipStream_t st) {
    long long* h = reinterpret_cast<long long*>(ctx->h_pinned);
    ASMC_HIP(hipMemcpyAsync(h, d_count, sizeof(long long), hipMemcpyDeviceToHost, st));
    ASMC_HIP(hipStreamSynchronize(st));
    *out_host = (int64_t)h[0];
    return ASMC_OK;
}

// count / scan / scatter of an ordered range selection; the number kept stays in scratch_count_total(ctx)
static int range_select_launch(asmc_ctx* ctx, int64_t n, const double* u_dev, const double* lohi_dev, double* out_dev, hipStream_t st) {
    const int64_t n_tiles = scan_tiles(n);
    ASMC_LAUNCH(ctx, st, "k_range_count", k_range_count, dim3((unsigned)n_tiles), dim3(ASMC_BLOCK), 0, st, n, u_dev, lohi_dev,
                ctx->d_tiles_i);
    ASMC_LAUNCH_CHECK();
    ASMC_LAUNCH(ctx, st, "k_scan_tiles_ll", k_scan_tiles_ll, dim3(1), dim3(64), 0, st, n_tiles, ctx->d_tiles_i, scratch_count_total(ctx));
    ASMC_LAUNCH_CHECK();
    ASMC_LAUNCH(ctx, st, "k_range_scatter", k_range_scatter<false>, dim3((unsigned)n_tiles), dim3(ASMC_BLOCK), 0, st, n, u_dev, lohi_dev,
                (const long long*)ctx->d_tiles_i, out_dev, (long long*)nullptr);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int asmc_range_select_shard_launch(asmc_ctx* ctx, int64_t n_u, const double* u_dev, const double* state_dev, const double* s_in,
                                   const double* cdf_last, double* edges_out_dev, double* out_dev, int64_t* info_dev, hipStream_t st) {
    const int64_t u_tiles = scan_tiles(n_u);
    ASMC_LAUNCH(ctx, st, "k_range_count_shard", k_range_count_shard, dim3((unsigned)u_tiles), dim3(ASMC_BLOCK), 0, st, n_u, u_dev,
                state_dev, s_in, cdf_last, ctx->d_tiles_i, edges_out_dev);
    ASMC_LAUNCH_CHECK();
    ASMC_LAUNCH(ctx, st, "k_range_scatter<scan>", k_range_scatter<true>, dim3((unsigned)u_tiles), dim3(ASMC_BLOCK), 0, st, n_u,
                u_dev, (const double*)(edges_out_dev + 2), (const long long*)ctx->d_tiles_i, out_dev,
                reinterpret_cast<long long*>(info_dev));
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

extern "C" {

int asmc_select_range(asmc_ctx* ctx, int64_t n, const double* u_dev, const double* lohi_dev, double* out_dev,
                      int64_t* count_host, asmc_stream stream) {
    ASMC_REQUIRE(ctx && u_dev && lohi_dev && out_dev && count_host, "null pointer");
    ASMC_REQUIRE(n > 0 && n <= ctx->n_max, "n out of range for this ctx");
    hipStream_t st = as_stream(stream);
    const int rc = range_select_launch(ctx, n, u_dev, lohi_dev, out_dev, st);
    if (rc) return rc;
    return read_back_count(ctx, scratch_count_total(ctx), count_host, st);
}

__global__ void k_range_info(const long long* __restrict__ total, const double* __restrict__ edges, long long* __restrict__ info) {
    info[0] = total[0];
    info[1] = (long long)llrint(edges[0]);
}

// asmc_select_range without the synchronisation: the count and the slice's failure flag (edges_dev[0], asmc_cdf_shard_finish)
// go to info_dev[0..1] (int64) - owner-layout resampling all-gathers them over the ranks and reads everything back at once
int asmc_select_range_dev(asmc_ctx* ctx, int64_t n, const double* u_dev, const double* edges_dev, double* out_dev,
                          int64_t* info_dev, asmc_stream stream) {
    ASMC_REQUIRE(ctx && u_dev && edges_dev && out_dev && info_dev, "null pointer");
    ASMC_REQUIRE(n > 0 && n <= ctx->n_max, "n out of range for this ctx");
    hipStream_t st = as_stream(stream);
    const int rc = range_select_launch(ctx, n, u_dev, edges_dev + 2, out_dev, st);
    if (rc) return rc;
    ASMC_LAUNCH(ctx, st, "k_range_info", k_range_info, dim3(1), dim3(1), 0, st, (const long long*)scratch_count_total(ctx), edges_dev,
                reinterpret_cast<long long*>(info_dev));
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

// jump table for this stream's increment: A_0 = MULT, C_0 = inc; A_{i+1} = A_i^2, C_{i+1} = (A_i+1) C_i
// (rebuilt only when the increment changes, i.e. when a different Generator is passed)
static int pcg_prepare(asmc_ctx* ctx, const uint64_t state_host[4], hipStream_t st) {
    if (!ctx->pcg_tab_valid || ctx->pcg_inc[0] != state_host[2] || ctx->pcg_inc[1] != state_host[3]) {
        unsigned long long* tab = reinterpret_cast<unsigned long long*>(ctx->h_pinned) + HP_PCG_TAB;
        ASMC_HIP(hipStreamSynchronize(st));  // pinned staging may still be in use by a previous call
        U128 A = {0x4385DF649FCCF645ULL, 0x2360ED051FC65DA4ULL};
        U128 C = {state_host[3], state_host[2]};
        for (int i = 0; i < 64; i++) {
            tab[4 * i] = A.lo;
            tab[4 * i + 1] = A.hi;
            tab[4 * i + 2] = C.lo;
            tab[4 * i + 3] = C.hi;
            U128 A1 = u128_add(A, U128{1ULL, 0ULL});
            C = u128_mul(A1, C);
            A = u128_mul(A, A);
        }
        ASMC_HIP(hipMemcpyAsync(ctx->d_pcgtab, tab, sizeof(unsigned long long) * 256, hipMemcpyHostToDevice, st));
        ASMC_HIP(hipStreamSynchronize(st));
        ctx->pcg_inc[0] = state_host[2];
        ctx->pcg_inc[1] = state_host[3];
        ctx->pcg_tab_valid = 1;
    }
    return ASMC_OK;
}

int asmc_pcg64_uniforms(asmc_ctx* ctx, const uint64_t state_host[4], uint64_t offset, int64_t n,
                        double* u, asmc_stream stream) {
    ASMC_REQUIRE(ctx && state_host && u, "null pointer");
    ASMC_REQUIRE(n > 0, "n must be positive");
    hipStream_t st = as_stream(stream);
    int rc = pcg_prepare(ctx, state_host, st);
    if (rc) return rc;
    U128 s0 = {state_host[1], state_host[0]};
    const int64_t threads = n < PCG_THREADS ? n : PCG_THREADS;
    const int grid = (int)((threads + ASMC_BLOCK - 1) / ASMC_BLOCK);
    ASMC_LAUNCH(ctx, st, "k_pcg64_uniforms", k_pcg64_uniforms, dim3(grid), dim3(ASMC_BLOCK), 0, st,
                       (const unsigned long long*)ctx->d_pcgtab, s0, (unsigned long long)offset, n, u);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int64_t asmc_pcg64_select_stage_len(int64_t n_total) {
    if (n_total <= 0) return 0;
    return ((n_total + ASMC_SELECT_THREADS - 1) / ASMC_SELECT_THREADS) * ASMC_SELECT_THREADS;
}

int asmc_pcg64_select(asmc_ctx* ctx, const uint64_t state_host[4], int64_t n_total, double lo, double hi,
                      double* stage, int64_t* count_host, asmc_stream stream) {
    ASMC_REQUIRE(ctx && state_host && stage && count_host, "null pointer");
    ASMC_REQUIRE(n_total > 0, "n_total must be positive");
    ASMC_REQUIRE(lo >= 0.0 && hi > lo && hi <= 1.0, "need 0 <= lo < hi <= 1");
    static_assert((1 << SEL_LOG2) == ASMC_SELECT_THREADS && SEL_WAVES % 1024 == 0, "select kernel geometry");
    hipStream_t st = as_stream(stream);
    int rc = pcg_prepare(ctx, state_host, st);
    if (rc) return rc;
    U128 s0 = {state_host[1], state_host[0]};
    const int64_t iters = (n_total + ASMC_SELECT_THREADS - 1) / ASMC_SELECT_THREADS;
    ASMC_LAUNCH(ctx, st, "k_pcg64_select", k_pcg64_select, dim3(ASMC_SELECT_THREADS / ASMC_BLOCK), dim3(ASMC_BLOCK), 0, st,
                (const unsigned long long*)ctx->d_pcgtab, s0, n_total, lo, hi, iters, stage, ctx->d_select);
    ASMC_LAUNCH_CHECK();
    ASMC_LAUNCH(ctx, st, "k_select_scan", k_select_scan, dim3(1), dim3(1024), 0, st, ctx->d_select);
    ASMC_LAUNCH_CHECK();
    return read_back_count(ctx, ctx->d_select + 2 * SEL_WAVES, count_host, st);
}

int asmc_pcg64_select_compact(asmc_ctx* ctx, int64_t n_total, const double* stage, double* q, asmc_stream stream) {
    ASMC_REQUIRE(ctx && stage && q, "null pointer");
    ASMC_REQUIRE(n_total > 0, "n_total must be positive");
    hipStream_t st = as_stream(stream);
    const int64_t iters = (n_total + ASMC_SELECT_THREADS - 1) / ASMC_SELECT_THREADS;
    ASMC_LAUNCH(ctx, st, "k_select_compact", k_select_compact, dim3(SEL_WAVES), dim3(64), 0, st, iters, stage,
                (const long long*)ctx->d_select, q);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int asmc_systematic_uniforms(asmc_ctx* ctx, int64_t n_out, int64_t j0, int64_t n_total, double u0,
                             const double* v, double* u, asmc_stream stream) {
    ASMC_REQUIRE(ctx && u, "null pointer");
    ASMC_REQUIRE(n_out > 0 && n_total > 0, "bad sizes");
    const int grid = grid_for(n_out, ASMC_BLOCK * 4, ASMC_MAX_BLOCKS);
    ASMC_LAUNCH(ctx, as_stream(stream), "k_systematic", k_systematic, dim3(grid), dim3(ASMC_BLOCK), 0, as_stream(stream), n_out, j0, n_total,
                       u0, v, u);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int asmc_search(asmc_ctx* ctx, int64_t n, const double* cdf, int64_t n_out, const double* u,
                int64_t* idx, asmc_stream stream) {
    ASMC_REQUIRE(ctx && cdf && u && idx, "null pointer");
    ASMC_REQUIRE(n > 0 && n_out > 0, "bad sizes");
    hipStream_t st = as_stream(stream);
    const int grid = grid_for(n_out, ASMC_BLOCK, ASMC_MAX_BLOCKS * 4);
    // guide table: one bucket per four cdf entries; worth building when the cdf no longer sits in L2 and there are
    // enough lookups to pay for the nb + 1 (cache-friendly) searches of the build
    static const bool no_guide = getenv("ASMC_SEARCH_PLAIN") != nullptr;
    const int64_t nb = n / 4;
    if (!no_guide && n >= (1 << 17) && n <= ctx->n_max && n < (1LL << 32) && n_out >= n / 8) {
        ASMC_LAUNCH(ctx, st, "k_guide_build", k_guide_build, dim3(grid_for(nb + 1, ASMC_BLOCK, ASMC_MAX_BLOCKS * 4)), dim3(ASMC_BLOCK), 0, st,
                    n, cdf, nb, ctx->d_guide);
        ASMC_LAUNCH_CHECK();
        ASMC_LAUNCH(ctx, st, "k_search", k_search_guided, dim3(grid), dim3(ASMC_BLOCK), 0, st, n, cdf, nb,
                    (const unsigned int*)ctx->d_guide, n_out, u, idx);
    } else {
        ASMC_LAUNCH(ctx, st, "k_search", k_search, dim3(grid), dim3(ASMC_BLOCK), 0, st, n, cdf, n_out, u, idx);
    }
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

// The sharded step's one synchronisation AND what follows it, without the host interpreter in between: waits for the chain
// (asmc_shard_step_result), and when the numbers read back are those of a finished step - search converged, no NaN weights,
// no slice that needs the replicated scan, every rank's offspring count in (0, cap]: conditions every rank evaluates on the same
// gathered values - puts this rank's search (asmc_search over its kept draws) and gather (asmc_gather into the caller's
// cap-row buffers; the records packed on the way are claimed by rec_token) onto the stream right away.  *launched = 1 then, and
// out_host[13 + 2 world + 2 rank] is the number of rows written.  The caller still takes resample_owner's decisions (shares,
// totals) from out_host and drops the rows if they say so.
int asmc_shard_step_finish(asmc_ctx* ctx, const double* res_dev, int world, int rank, int64_t n_local, const double* cdf_dev,
                           const double* kept_dev, int64_t cap, int64_t* idx_dev, int d, int x_dtype, const void* x_in,
                           void* x_out, const double* ll_in, const double* lp_in, const double* lq_in, double* ll_out,
                           double* lp_out, double* lq_out, int64_t rec_token, double* out_host, int* launched,
                           asmc_stream stream) {
    ASMC_REQUIRE(ctx && res_dev && cdf_dev && kept_dev && idx_dev && x_in && x_out && ll_in && lp_in && lq_in && ll_out && lp_out &&
                     lq_out && out_host && launched,
                 "null pointer");
    ASMC_REQUIRE(world >= 1 && rank >= 0 && rank < world && n_local > 0 && cap > 0 && d > 0, "bad sizes");
    *launched = 0;
    int rc = asmc_shard_step_result(ctx, res_dev, world, out_host, stream);
    if (rc) return rc;
    const double* info = out_host + 13 + 2 * world;  // (kept, fail) per rank, as doubles
    bool usable = out_host[2] != 0.0 && out_host[5] == 0.0 && out_host[9] != 0.0;
    for (int r = 0; r < world && usable; r++) usable = info[2 * r + 1] == 0.0 && info[2 * r] > 0.0 && info[2 * r] <= (double)cap;
    if (!usable) return ASMC_OK;
    const int64_t cnt = (int64_t)info[2 * rank];
    rc = asmc_search(ctx, n_local, cdf_dev, cnt, kept_dev, idx_dev, stream);
    if (rc) return rc;
    (void)asmc_rec_claim(ctx, rec_token, n_local, ll_in, lp_in, lq_in);
    rc = asmc_gather(ctx, n_local, cnt, idx_dev, d, x_dtype, x_in, x_out, ll_in, lp_in, lq_in, ll_out, lp_out, lq_out, stream);
    if (rc) return rc;
    *launched = 1;
    return ASMC_OK;
}

int asmc_importance_step(asmc_ctx* ctx, int64_t n, const double* ll, const double* lp, const double* lq, double beta0,
                         double target_eff, double tol, const uint64_t rng_state[4], int64_t n_out, double* w_scratch,
                         double* cdf_scratch, int64_t* idx_out, asmc_stream stream) {
    ASMC_REQUIRE(ctx && ll && lp && lq && rng_state && w_scratch && cdf_scratch && idx_out, "null pointer");
    ASMC_REQUIRE(n > 0 && n <= ctx->n_max && n < (1LL << 32) && n_out > 0, "bad sizes");
    ASMC_REQUIRE(tol > 0.0 && beta0 >= 0.0 && beta0 < 1.0, "bad beta0 / tolerance");
    hipStream_t st = as_stream(stream);
    // jump table of the generator's increment (host work + one upload, only when the increment changes)
    int rc = pcg_prepare(ctx, rng_state, st);
    if (rc) return rc;
    // 1: beta search, evidence moments, normalised weights, tile sums (one persistent launch)
    // (the kernel also leaves the (ll, lp, lq, 0) records of asmc_gather in ctx->d_rec: tagged at the end of this call)
    static const bool no_rec = getenv("ASMC_IS_NO_RECORDS") != nullptr;
    rc = asmc_is_weights_launch(ctx, n, ll, lp, lq, beta0, target_eff, tol, w_scratch, ctx->d_tiles, no_rec ? nullptr : ctx->d_rec, st);
    if (rc) return rc;
    if (!no_rec) ctx->rec_token++;  // (d_rec rewritten)
    // 2-4: numpy's sequential cumsum and the division by its last entry (passes C, D, E of asmc_cdf, asmc_cdf.hip; the tile prefixes ride on pass C
    // while there are few tiles), pass E also filling the search's guide table
    static const bool no_guide = getenv("ASMC_SEARCH_PLAIN") != nullptr;
    // one bucket per cdf entry (round 5; n / 4 before): a lookup is then the guide's pair and 1 - 2 dependent cdf reads instead
    // of ~3 - the search is bound by its random requests (fetching whole 64-byte windows instead of bisecting doubled its time) -
    // 34.6 -> 26.2 us at 1M, 430 -> 281 us at 8M, for + 1.3 / + 7 us of table fill in pass E.  2 n buckets gain nothing more at 1M.
    const int64_t nb = n;
    const bool guided = !no_guide && n >= (1 << 17) && n_out >= n / 8;
    rc = asmc_exact_cdf_enqueue(ctx, n, w_scratch, cdf_scratch, XCDF_HAVE_SUMS, 0.0, nullptr, 1, nullptr, ctx->d_small + DS_CDF_TOTAL,
                                guided ? ctx->d_guide : (unsigned int*)nullptr, nb, st);
    if (rc) return rc;
    // 5: rng.random(n_out) and searchsorted(cdf, u, side="right") in one pass
    int tlog2 = SP_LOG2;
    while (tlog2 > 6 && ((int64_t)1 << (tlog2 - 1)) >= n_out) tlog2--;
    const int64_t threads = (int64_t)1 << tlog2;
    U128 s0 = {rng_state[1], rng_state[0]};
    ASMC_LAUNCH(ctx, st, "k_search_pcg", k_search_pcg, dim3((unsigned)((threads + ASMC_BLOCK - 1) / ASMC_BLOCK)), dim3(ASMC_BLOCK), 0, st,
                (const unsigned long long*)ctx->d_pcgtab, s0, tlog2, n, (const double*)cdf_scratch, nb,
                guided ? (const unsigned int*)ctx->d_guide : (const unsigned int*)nullptr, n_out, idx_out);
    ASMC_LAUNCH_CHECK();
    if (!no_rec) ctx->rec_src[0] = ll, ctx->rec_src[1] = lp, ctx->rec_src[2] = lq, ctx->rec_n = n;  // (any later launch clears it)
    return ASMC_OK;
}

// The (ll, lp, lq, 0) records that asmc_normalized_weights_shard packed on its way (pack_records = 1) become the next asmc_gather's
// records if `token` (asmc_rec_token right after that call) is still d_rec's generation, i.e. no other pass has rewritten d_rec
// since, and the arrays are the ones packed.  Returns 1 when claimed, 0 otherwise (the gather then packs for itself).  Call it
// directly in front of asmc_gather: any launch in between drops the claim again.
int64_t asmc_rec_token(asmc_ctx* ctx) { return ctx ? (int64_t)ctx->rec_token : -1; }
int asmc_rec_claim(asmc_ctx* ctx, int64_t token, int64_t n, const double* ll, const double* lp, const double* lq) {
    if (!ctx || token <= 0 || (uint64_t)token != ctx->rec_token || ctx->rec_hold_token != (uint64_t)token || ctx->rec_hold_n != n ||
        ctx->rec_hold_src[0] != ll || ctx->rec_hold_src[1] != lp || ctx->rec_hold_src[2] != lq)
        return 0;
    ctx->rec_src[0] = ll, ctx->rec_src[1] = lp, ctx->rec_src[2] = lq, ctx->rec_n = n;
    return 1;
}

int asmc_gather(asmc_ctx* ctx, int64_t n_in, int64_t n_out, const int64_t* idx, int d, int x_dtype, const void* x_in,
                void* x_out, const double* ll_in, const double* lp_in, const double* lq_in,
                double* ll_out, double* lp_out, double* lq_out, asmc_stream stream) {
    ASMC_REQUIRE(ctx && idx && x_in && x_out && ll_in && lp_in && lq_in && ll_out && lp_out && lq_out,
                 "null pointer");
    ASMC_REQUIRE(n_in > 0 && n_out > 0 && d > 0, "bad sizes");
    ASMC_REQUIRE(x_dtype == ASMC_F64 || x_dtype == ASMC_F32, "bad x_dtype");
    hipStream_t st = as_stream(stream);
    const LogRec* rec = nullptr;
    if (ctx->rec_n == n_in && ctx->rec_src[0] == ll_in && ctx->rec_src[1] == lp_in && ctx->rec_src[2] == lq_in) {
        rec = reinterpret_cast<const LogRec*>(ctx->d_rec);  // packed by the importance step that selected these draws
    } else if (n_in <= ctx->n_max && n_out >= n_in / 4 && n_in >= (1 << 16)) {  // enough draws to pay for the packing pass
        LogRec* r = reinterpret_cast<LogRec*>(ctx->d_rec);
        ASMC_LAUNCH(ctx, st, "k_pack_records", k_pack_records, dim3(grid_for(n_in, ASMC_BLOCK * 2, ASMC_MAX_BLOCKS * 2)), dim3(ASMC_BLOCK), 0, st,
                    n_in, ll_in, lp_in, lq_in, r);
        ASMC_LAUNCH_CHECK();
        ctx->rec_token++;  // (d_rec rewritten)
        rec = r;
    }
    const size_t elem = x_dtype == ASMC_F64 ? 8 : 4;
    const size_t rowbytes = elem * (size_t)d;
    const bool vec_ok = (rowbytes % 16 == 0) && (((uintptr_t)x_in | (uintptr_t)x_out) % 16 == 0);
    if (vec_ok) {
        const int cpr = (int)(rowbytes / 16);
        const int grid = grid_for(n_out * cpr, ASMC_BLOCK * 4, ASMC_MAX_BLOCKS * 2);
        static const bool plain_gather = getenv("ASMC_GATHER_PLAIN") != nullptr;
        bool cs_done = false;
        // fp64 rows of a width the moment kernels take: the column sums of the gathered rows ride along (tagged below)
        const bool cs = x_dtype == ASMC_F64 && (d == 32 || d == 64 || d == 16) && (size_t)grid * d <= ctx->gram_cap &&
                        !getenv("ASMC_GATHER_NO_COLSUM");
#define ASMC_GATHER_POW2(SHV)                                                                                       \
    if (!plain_gather && cpr == (1 << SHV)) {                                                                      \
        if (cs)                                                                                                    \
            ASMC_LAUNCH(ctx, st, "k_gather16", (k_gather16_pow2<SHV, true>), dim3(grid), dim3(ASMC_BLOCK), 0, st, n_out, idx, \
                        rec, (const uint4*)x_in, (uint4*)x_out, ll_in, lp_in, lq_in, ll_out, lp_out, lq_out, ctx->d_gram);  \
        else                                                                                                       \
            ASMC_LAUNCH(ctx, st, "k_gather16", (k_gather16_pow2<SHV, false>), dim3(grid), dim3(ASMC_BLOCK), 0, st, n_out, idx, \
                        rec, (const uint4*)x_in, (uint4*)x_out, ll_in, lp_in, lq_in, ll_out, lp_out, lq_out, (double*)nullptr); \
        cs_done = cs;                                                                                              \
    } else
        ASMC_GATHER_POW2(4)
        ASMC_GATHER_POW2(3)
        ASMC_GATHER_POW2(5)
        {
    ASMC_LAUNCH(ctx, st, "k_gather16", k_gather16, dim3(grid), dim3(ASMC_BLOCK), 0, st, n_out, idx, rec, cpr,
                           (const uint4*)x_in, (uint4*)x_out, ll_in, lp_in, lq_in, ll_out, lp_out, lq_out);
        }
#undef ASMC_GATHER_POW2
        // (any later launch drops the tag: the partials live in the moment kernels' scratch)
        if (cs_done) ctx->cs_x = x_out, ctx->cs_n = n_out, ctx->cs_d = d, ctx->cs_grid = grid;
    } else if (x_dtype == ASMC_F64) {
        const int grid = grid_for(n_out * d, ASMC_BLOCK * 4, ASMC_MAX_BLOCKS * 2);
        ASMC_LAUNCH(ctx, st, "k_gather_elem<double>", k_gather_elem<double>, dim3(grid), dim3(ASMC_BLOCK), 0, st, n_out, idx, rec, d,
                           (const double*)x_in, (double*)x_out, ll_in, lp_in, lq_in, ll_out, lp_out, lq_out);
    } else {
        const int grid = grid_for(n_out * d, ASMC_BLOCK * 4, ASMC_MAX_BLOCKS * 2);
        ASMC_LAUNCH(ctx, st, "k_gather_elem<float>", k_gather_elem<float>, dim3(grid), dim3(ASMC_BLOCK), 0, st, n_out, idx, rec, d,
                           (const float*)x_in, (float*)x_out, ll_in, lp_in, lq_in, ll_out, lp_out, lq_out);
    }
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int asmc_compact_valid(asmc_ctx* ctx, int64_t n, int d, int x_dtype, const void* x, const double* ll,
                       const double* lp, const double* lq, void* x_out, double* ll_out, double* lp_out,
                       double* lq_out, int64_t* n_valid_host, asmc_stream stream) {
    ASMC_REQUIRE(ctx && x && ll && lp && lq && x_out && ll_out && lp_out && lq_out && n_valid_host,
                 "null pointer");
    ASMC_REQUIRE(n > 0 && n <= ctx->n_max && d > 0, "bad sizes");
    ASMC_REQUIRE(x_dtype == ASMC_F64 || x_dtype == ASMC_F32, "bad x_dtype");
    hipStream_t st = as_stream(stream);
    const int64_t n_tiles = scan_tiles(n);
    long long* d_total = scratch_count_total(ctx);
    ASMC_LAUNCH(ctx, st, "k_valid_count", k_valid_count, dim3((unsigned)n_tiles), dim3(ASMC_BLOCK), 0, st, n, ll, lp, ctx->d_tiles_i);
    ASMC_LAUNCH_CHECK();
    ASMC_LAUNCH(ctx, st, "k_scan_tiles_ll", k_scan_tiles_ll, dim3(1), dim3(64), 0, st, n_tiles, ctx->d_tiles_i, d_total);
    ASMC_LAUNCH_CHECK();
    const int rc = read_back_count(ctx, d_total, n_valid_host, st);
    if (rc) return rc;
    if (*n_valid_host == n) return ASMC_OK;  // already compact (the usual case): nothing is copied, the caller keeps its inputs
    if (x_dtype == ASMC_F64)
        ASMC_LAUNCH(ctx, st, "k_compact_scatter<double>", k_compact_scatter<double>, dim3((unsigned)n_tiles), dim3(ASMC_BLOCK), 0, st, n, d,
                           (const double*)x, ll, lp, lq, (const long long*)ctx->d_tiles_i, (double*)x_out,
                           ll_out, lp_out, lq_out);
    else
        ASMC_LAUNCH(ctx, st, "k_compact_scatter<float>", k_compact_scatter<float>, dim3((unsigned)n_tiles), dim3(ASMC_BLOCK), 0, st, n, d,
                           (const float*)x, ll, lp, lq, (const long long*)ctx->d_tiles_i, (float*)x_out,
                           ll_out, lp_out, lq_out);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

}  // extern "C"
