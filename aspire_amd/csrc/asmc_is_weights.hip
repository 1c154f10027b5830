// asmc_is_weights.hip — the importance step's weight half in one persistent launch: k_is_weights and its grid barrier, the launcher
// asmc_importance_step enqueues (asmc_is_weights_launch) and the calls that read its results back.
// The search rounds inside it are k_bis_sums' (asmc_search.hip), on resident particles; what the two share: asmc_search_dev.h.
#include "asmc_search_dev.h"

// ---------------------------------------------------------------------------------------------------------------
// The importance step's weight half in ONE persistent launch (asmc_importance_weights; smc/base.py:167-186 followed by
// samples.py:1230-1249 and :1276-1277): exact maximum at beta = 1 and the NaN census, the k-ary search rounds of
// k_bis_sums, the evidence-variance / second log-sum-exp pass of k_weights_m2_lse and the normalised weights with the
// scan's tile sums.  One block per CU, every block resident (the launch asks for no more blocks than CUs), the phases
// separated by grid barriers on a counter that only grows (no memset node; the launch's budget of ISW_BARRIERS
// arrivals per block is topped up at the end so that the next launch's base is where the counter stands).  A block
// owns a contiguous range of whole 4096-particle chunks (two scan tiles); REG: one chunk per block, the particles'
// (ll + lp, lq) stay in registers across all phases, so HBM/L2 is read once instead of once per round.
// Every block closes a round redundantly from the same partial records (fixed order => the same bits everywhere):
// no block waits for another one's decision, and the state record never leaves LDS between rounds.
// Results: st_out[0 .. BIS_STATE_LEN) = the search record (asmc_bisect.h), then the ISW_OUT_* cells below.
#define ISW_THREADS 512
#define ISW_PER 8
#define ISW_CHUNK (ISW_THREADS * ISW_PER)
#define ISW_MAX_ROUNDS 20
#define ISW_BARRIERS 32

// Two-level arrival: block b counts in on the counter of its group b % ISW_GROUPS (the counters sit in different
// memory channels, so the same-address atomics of one arrival wave serialise 8-fold less); the last block of a group
// counts the group in on the top counter, which everybody polls with plain device-scope loads.
// bar: [0] top counter, [ISW_BAR_STRIDE * (1 + g)] group g; bases: their values when this launch started.
// k_is_weights' result record (ctx->d_small + DS_BISECT): the state record, then
enum {
    ISW_OUT_M2 = BIS_STATE_LEN,  // sum (exp(lw - m) - mean_u)^2
    ISW_OUT_S1P = 41,            // S1'
    ISW_OUT_LSE = 42,            // lse'
    ISW_OUT_SHIFT = 43,
    ISW_OUT_MP = 44,
    ISW_OUT_FOUND = 45,          // 1 when beta* was found and w / tile sums are those of beta* (otherwise w = 1/N)
    ISW_OUT_STAMPS = 48,         // ISW_STAMP builds: 16 time stamps of block 0
    ISW_OUT_LEN = 64             // what the result calls copy out (= DS_BISECT_REC)
};
static_assert(ISW_OUT_M2 == 40 && ISW_OUT_STAMPS + 16 <= ISW_OUT_LEN && ISW_OUT_LEN == DS_BISECT_REC, "result cells behind the state record");

// (ISW_GROUPS, ISW_BAR_STRIDE, ISW_POISON_CELL: the map of ctx->d_bar in asmc_scratch.h)
struct IswBases {
    unsigned int top, group[ISW_GROUPS];
};
// Returns false when the other blocks did not arrive within ~0.5 s: the launch was not fully resident (two such kernels
// of different processes sharing the GPU can each hold half of the CUs).  The caller then abandons the search - uniform
// weights, found = 0 - and raises the poison cell; the host resets the counters and stops using this kernel.
#define ISW_SPIN_LIMIT (1 << 18)
__device__ __forceinline__ bool isw_barrier(unsigned int* bar, const IswBases& bases, unsigned int k, int G) {
    __shared__ int s_ok;
    // only wave 0 writes what the other blocks read behind the barrier (partial records, block maxima): the other waves'
    // stores (the gather's records, the weights) need not have landed
    if (threadIdx.x < 64) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const int g = blockIdx.x % ISW_GROUPS;
        const unsigned int ngroups = G < ISW_GROUPS ? G : ISW_GROUPS;
        const unsigned int gsize = (unsigned int)(G - g + ISW_GROUPS - 1) / ISW_GROUPS;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const unsigned int old = __hip_atomic_fetch_add(bar + ISW_BAR_STRIDE * (1 + g), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old - bases.group[g] == k * gsize - 1u)  // this block completes its group's k-th arrival
            __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned int target = bases.top + k * ngroups;
        int spins = 0;
        while ((int)(__hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) < 0 && spins < ISW_SPIN_LIMIT) {
            __builtin_amdgcn_s_sleep(1);
            spins++;
        }
        s_ok = spins < ISW_SPIN_LIMIT;
        if (!s_ok) __hip_atomic_store(bar + ISW_POISON_CELL, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
    return s_ok != 0;
}

template <bool REG>
__global__ __launch_bounds__(ISW_THREADS) void k_is_weights(int64_t n, const double* __restrict__ ll,
                                                           const double* __restrict__ lp, const double* __restrict__ lq,
                                                           double* __restrict__ st_out, double* partials,
                                                           unsigned int* bar, IswBases bar_bases, BisInit init,
                                                           int64_t chunk, double* __restrict__ w,
                                                           double* __restrict__ tiles, double* __restrict__ rec) {
    __shared__ BisLds L;
    __shared__ double s_red[ISW_THREADS / 32][33];
    __shared__ double s_S[32];
    __shared__ double s_eff[16];
    __shared__ double s_p[ISW_THREADS / 64][32];
    __shared__ double s_sc[8];
    __shared__ double s_base[ISW_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, G = (int)gridDim.x;
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = (lo + chunk < n) ? lo + chunk : n;
    const int nsub = (int)(chunk / ISW_CHUNK);
    unsigned int nbar = 0;
#ifdef ISW_STAMP
    const unsigned long long t_start = wall_clock64();
    int n_stamp = 0;
    double stamps[16];
#define ISW_MARK()                                                                         \
    do {                                                                                   \
        if (n_stamp < 16) stamps[n_stamp++] = (double)(wall_clock64() - t_start) * 0.01; \
    } while (0)
#else
#define ISW_MARK() \
    do {           \
    } while (0)
#endif
    bool poisoned = false;  // a barrier timed out: finish with uniform weights (see isw_barrier)
    auto barrier = [&]() {
        if (poisoned) return;
        nbar++;
        poisoned = !isw_barrier(bar, bar_bases, nbar, G);
    };
    auto pbuf = [&](unsigned int k) { return partials + (size_t)(k & 1u) * (size_t)G * 32; };
    double* mrec = partials + (size_t)2 * G * 32;  // (maximum, NaN count) of every block

    // REG: the block's particles as (ll + lp, lq) in LDS, staged once (64 KB of dynamic LDS)
    extern __shared__ double s_part[];
    double* s_ab = s_part;
    double* s_q = s_part + ISW_CHUNK;
    if (REG) {
#pragma unroll
        for (int k = 0; k < ISW_PER; k++) {
            const int64_t i = lo + k * ISW_THREADS + tid;
            const bool ok = i < hi;
            const double a = ok ? ll[i] : 0.0, b = ok ? lp[i] : 0.0, q = ok ? lq[i] : 0.0;
            s_ab[k * ISW_THREADS + tid] = a + b;
            s_q[k * ISW_THREADS + tid] = q;
            // the (ll, lp, lq, 0) record asmc_gather reads per draw (k_pack_records' job, done on the way)
            if (rec && ok) *reinterpret_cast<double4*>(rec + 4 * i) = make_double4(a, b, q, 0.0);
        }
        // every thread only ever reads back its own entries: no barrier needed
    }
    // particle k of sub-chunk `sub` of this thread: (ll + lp, lq); false behind the end of the block's range
    auto get = [&](int sub, int k, double& abv, double& qv) {
        const int64_t i = lo + (int64_t)sub * ISW_CHUNK + k * ISW_THREADS + tid;
        const bool ok = i < hi;
        if (REG) {
            abv = s_ab[k * ISW_THREADS + tid];
            qv = s_q[k * ISW_THREADS + tid];
        } else {
            const double a = ok ? ll[i] : 0.0, b = ok ? lp[i] : 0.0;
            abv = a + b;
            qv = ok ? lq[i] : 0.0;
        }
        return ok;
    };
    // the reference's log-weight (samples.py:1222-1224) from ll + lp and lq
    auto lw_at = [&](double abv, double qv, double c1, double c2) {
        const double t1 = c1 * qv;
        const double t2 = c2 * abv;
        return t1 + t2;
    };

    // ---- phase 0: THIS BLOCK's maximum of the log-weights at beta = 1 and its NaN census (no grid barrier: the first
    // search round shifts by the block's own maximum and the round's reduction rescales to the merged one) -------------
    {
        const double c1 = init.beta0 - 1.0, c2 = 1.0 - init.beta0;
        double mx = -INFINITY;
        long long nn = 0;
        for (int sub = 0; sub < nsub; sub++) {
#pragma unroll 4
            for (int k = 0; k < ISW_PER; k++) {
                double abv, qv;
                bool ok;
                if (REG) {
                    ok = get(sub, k, abv, qv);
                } else {  // streaming: the records are packed from this first read
                    const int64_t i = lo + (int64_t)sub * ISW_CHUNK + k * ISW_THREADS + tid;
                    ok = i < hi;
                    const double a = ok ? ll[i] : 0.0, b = ok ? lp[i] : 0.0;
                    abv = a + b, qv = ok ? lq[i] : 0.0;
                    if (rec && ok) *reinterpret_cast<double4*>(rec + 4 * i) = make_double4(a, b, qv, 0.0);
                }
                if (ok) {
                    const double lw = lw_at(abv, qv, c1, c2);
                    if (lw != lw)
                        nn++;
                    else
                        mx = fmax(mx, lw);
                }
            }
        }
        mx = wave_max(mx);
        nn = wave_sum_ll(nn);
        if (lane == 0) s_p[wave][0] = mx, s_p[wave][1] = (double)nn;
        __syncthreads();
        if (tid == 0) {
            double v = s_p[0][0], c = s_p[0][1];
            for (int x = 1; x < ISW_THREADS / 64; x++) v = fmax(v, s_p[x][0]), c += s_p[x][1];
            s_sc[0] = v, s_sc[1] = c;
            mrec[2 * blockIdx.x] = v, mrec[2 * blockIdx.x + 1] = c;
        }
        __syncthreads();
        ISW_MARK();
    }
    const double m_block = s_sc[0] > -INFINITY ? s_sc[0] : 0.0;  // (no finite log-weight in the block: its sums are zero)
    double m_one = 0.0, nan_total = 0.0;
    bis_lds_init(L, init, 0.0, 0.0);  // (a poisoned first barrier leaves the loop before the record is created)

    // ---- phase 1: the search rounds (k_bis_sums on the resident particles) ------------------------------------------
    for (int round = 0; round < ISW_MAX_ROUNDS; round++) {
        BisGrid g;
        if (round == 0)
            g = bis_first_grid(init.beta0, m_block);
        else
            g = bis_next_grid(L.st);
        double s1[16], s2[16];
#pragma unroll
        for (int j = 0; j < 16; j++) s1[j] = 0.0, s2[j] = 0.0;
        for (int sub = 0; sub < nsub; sub++) {
#pragma unroll 1
            for (int k = 0; k < ISW_PER; k += 2) {  // two particles per trip (k_bis_sums)
                double ab0, q0, ab1, q1;
                const bool v0 = get(sub, k, ab0, q0), v1 = get(sub, k + 1, ab1, q1);
                const double e = v0 ? exp(lw_at(ab0, q0, g.c1, g.c2) - g.m1) : 0.0;
                const double r = v0 ? exp(g.h * ((ab0 - q0) - g.dmax)) : 0.0;
                const double e2 = v1 ? exp(lw_at(ab1, q1, g.c1, g.c2) - g.m1) : 0.0;
                const double r2 = v1 ? exp(g.h * ((ab1 - q1) - g.dmax)) : 0.0;
                bis_accumulate(s1, s2, e, r, e2, r2);
            }
        }
        // bis_block_record (asmc_search_dev.h) written out (why: docs/changelog.md); keep the two in step
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
        double* buf = pbuf(nbar + 1);
        if (tid < 32) {
            double v = s_p[0][tid];
            for (int x = 1; x < ISW_THREADS / 64; x++) v += s_p[x][tid];
            buf[(size_t)blockIdx.x * 32 + tid] = v;
        }
        ISW_MARK();
        barrier();
        if (poisoned) break;
        ISW_MARK();
        if (round == 0) {
            // merged maximum and NaN census of the blocks and the records rescaled to it; this creates the state record
            bis_reduce_partials_scaled(buf, mrec, G, s_red, s_S, s_base, s_sc);
            __syncthreads();
            m_one = s_sc[0], nan_total = s_sc[1];
            bis_lds_init(L, init, m_one, nan_total);
        } else {
            bis_reduce_partials(buf, G, s_red, s_S);
        }
        __syncthreads();
        bis_tail_core(L, round == 0, s_S, s_eff);
        ISW_MARK();
        if (L.st[BIS_DONE] != 0.0) break;  // uniform: every block took the same decisions
    }

    // ---- phase 2: evidence variance + second log-sum-exp at beta*, then the normalised weights -----------------------
    const double beta0 = init.beta0, beta = L.st[BIS_BMIN], N = init.N;
    bool found = !poisoned && L.st[BIS_DONE] != 0.0 && L.st[BIS_TRIP_OK] != 0.0 && nan_total == 0.0 && beta > beta0;
    const double c1 = beta0 - beta, c2 = beta - beta0;
    const int64_t n_tiles = (n + ASMC_SCAN_TILE - 1) / ASMC_SCAN_TILE;
    double shift = 0.0, mp = 0.0, lse = 0.0;
    if (found) {
        // smc_math.evidence_variance_and_lse's scalars, same operation order
        const double m = L.st[BIS_TRIP_M], S1 = L.st[BIS_TRIP_S1];
        const double mean_u = S1 / N;
        shift = (m + log(S1)) - init.logN;
        mp = m + shift;
        double acc = 0.0, s1p = 0.0;
        for (int sub = 0; sub < nsub; sub++) {
#pragma unroll 2
            for (int k = 0; k < ISW_PER; k++) {
                double abv, qv;
                if (get(sub, k, abv, qv)) {
                    const double lw = lw_at(abv, qv, c1, c2);
                    const double dlt = exp(lw - m) - mean_u;
                    acc += dlt * dlt;
                    s1p += exp((lw + shift) - mp);
                }
            }
        }
        acc = wave_sum(acc);
        s1p = wave_sum(s1p);
        __syncthreads();
        if (lane == 0) s_p[wave][0] = acc, s_p[wave][1] = s1p;
        __syncthreads();
        double* buf = pbuf(nbar + 1);
        if (tid < 2) {
            double v = s_p[0][tid];
            for (int x = 1; x < ISW_THREADS / 64; x++) v += s_p[x][tid];
            buf[(size_t)blockIdx.x * 32 + tid] = v;
        }
        barrier();
        if (tid < 64) {  // k_finalize_columns' order: 64 strided chains, then the wave butterfly
            double v0 = 0.0, v1 = 0.0;
            for (int b = tid; b < G; b += 64) {
                v0 += buf[(size_t)b * 32];
                v1 += buf[(size_t)b * 32 + 1];
            }
            v0 = wave_sum(v0);
            v1 = wave_sum(v1);
            if (tid == 0) s_sc[2] = v0, s_sc[3] = v1, s_sc[4] = mp + log(v1);  // lse' = mp + log S1'
        }
        __syncthreads();
        lse = s_sc[4];
        if (poisoned) found = false;
    }
    const double w_uniform = 1.0 / N;
    for (int sub = 0; sub < nsub; sub++) {
        double ts0 = 0.0, ts1 = 0.0;
#pragma unroll 2
        for (int k = 0; k < ISW_PER; k++) {
            double abv, qv;
            if (get(sub, k, abv, qv)) {
                const double wv = found ? exp((lw_at(abv, qv, c1, c2) + shift) - lse) : w_uniform;
                w[lo + (int64_t)sub * ISW_CHUNK + k * ISW_THREADS + tid] = wv;
                if (k < ISW_PER / 2)
                    ts0 += wv;
                else
                    ts1 += wv;
            }
        }
        ts0 = wave_sum(ts0);
        ts1 = wave_sum(ts1);
        __syncthreads();
        if (lane == 0) s_p[wave][0] = ts0, s_p[wave][1] = ts1;
        __syncthreads();
        if (tid < 2) {
            double v = s_p[0][tid];
            for (int x = 1; x < ISW_THREADS / 64; x++) v += s_p[x][tid];
            const int64_t t = (lo + (int64_t)sub * ISW_CHUNK) / ASMC_SCAN_TILE + tid;
            if (t < n_tiles) tiles[t] = v;
        }
    }
    if (blockIdx.x == 0) {
        if (tid < BIS_STATE_LEN) st_out[tid] = L.st[tid];
        if (tid == ISW_OUT_M2) st_out[ISW_OUT_M2] = found ? s_sc[2] : 0.0;
        if (tid == ISW_OUT_S1P) st_out[ISW_OUT_S1P] = found ? s_sc[3] : 0.0;
        if (tid == ISW_OUT_LSE) st_out[ISW_OUT_LSE] = lse;
        if (tid == ISW_OUT_SHIFT) st_out[ISW_OUT_SHIFT] = shift;
        if (tid == ISW_OUT_MP) st_out[ISW_OUT_MP] = mp;
        if (tid == ISW_OUT_FOUND) st_out[ISW_OUT_FOUND] = found ? 1.0 : 0.0;
#ifdef ISW_STAMP
        ISW_MARK();
        if (tid == 0)
            for (int k = 0; k < 16; k++) st_out[ISW_OUT_STAMPS + k] = k < n_stamp ? stamps[k] : -1.0;
#endif
        // top the counters up to this launch's budget: the next launch's bases
        const unsigned int left = poisoned ? 0u : (unsigned int)(ISW_BARRIERS - nbar);  // (poisoned: the host resets them)
        if (tid == 0) __hip_atomic_fetch_add(bar, left * (unsigned int)(G < ISW_GROUPS ? G : ISW_GROUPS), __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
        if (tid >= 1 && tid <= ISW_GROUPS && tid - 1 < G) {
            const int g = tid - 1;
            __hip_atomic_fetch_add(bar + ISW_BAR_STRIDE * (1 + g), left * ((unsigned int)(G - g + ISW_GROUPS - 1) / ISW_GROUPS),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

int asmc_is_weights_launch(asmc_ctx* ctx, int64_t n, const double* ll, const double* lp, const double* lq, double beta0,
                           double target_eff, double tol, double* w, double* tiles, double* rec, hipStream_t st) {
    if (ctx->isw_disabled) {
        asmc_set_error("asmc_importance_step: disabled on this context (an earlier launch was not fully resident)");
        return ASMC_ERR_UNSUPPORTED;
    }
    const BisInit init = bis_init(beta0, target_eff, tol, n);
    int64_t chunk = ISW_CHUNK;
    int64_t grid = (n + chunk - 1) / chunk;
    ASMC_REQUIRE(ctx->num_cu <= ISW_THREADS, "more compute units than the first round's reduction has threads");
    const bool reg = grid <= ctx->num_cu;
    if (!reg) {
        chunk = (n + ctx->num_cu - 1) / ctx->num_cu;
        chunk = (chunk + ISW_CHUNK - 1) / ISW_CHUNK * ISW_CHUNK;
        grid = (n + chunk - 1) / chunk;
    }
    double* d_st = ctx->d_small + DS_BISECT;
    IswBases bases;
    bases.top = ctx->bar_base[0];
    if (getenv("ASMC_ISW_TEST_TIMEOUT")) bases.top += 1000000u;  // test hook: the barriers of this launch can never complete
    ctx->bar_base[0] += (unsigned int)ISW_BARRIERS * (unsigned int)(grid < ISW_GROUPS ? grid : ISW_GROUPS);
    for (int g = 0; g < ISW_GROUPS; g++) {
        bases.group[g] = ctx->bar_base[1 + g];
        if (g < grid) ctx->bar_base[1 + g] += (unsigned int)ISW_BARRIERS * (unsigned int)((grid - g + ISW_GROUPS - 1) / ISW_GROUPS);
    }
    if (reg) {
        static bool attr_set_dev[ASMC_MAX_DEVICES] = {false}; bool& attr_set = attr_set_dev[asmc_dev_slot(ctx)];
        if (!attr_set) {
            ASMC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_is_weights<true>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, 2 * ISW_CHUNK * (int)sizeof(double)));
            attr_set = true;
        }
        ASMC_LAUNCH(ctx, st, "k_is_weights", k_is_weights<true>, dim3((unsigned)grid), dim3(ISW_THREADS),
                    2 * ISW_CHUNK * sizeof(double), st, n, ll, lp, lq, d_st,
                    ctx->d_partials, ctx->d_bar, bases, init, chunk, w, tiles, rec);
    } else {
        ASMC_LAUNCH(ctx, st, "k_is_weights", k_is_weights<false>, dim3((unsigned)grid), dim3(ISW_THREADS), 0, st, n, ll, lp, lq, d_st,
                    ctx->d_partials, ctx->d_bar, bases, init, chunk, w, tiles, rec);
    }
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

// the result record and the poison word -> HP_STEP_RESULT (asmc_scratch.h), enqueued only
static int isw_readback_enqueue(asmc_ctx* ctx, hipStream_t st) {
    double* h = ctx->h_pinned + HP_STEP_RESULT;
    unsigned int* hp = reinterpret_cast<unsigned int*>(h + ISW_OUT_LEN);
    ASMC_HIP(hipMemcpyAsync(h, ctx->d_small + DS_BISECT, sizeof(double) * ISW_OUT_LEN, hipMemcpyDeviceToHost, st));
    ASMC_HIP(hipMemcpyAsync(hp, ctx->d_bar + ISW_POISON_CELL, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    return ASMC_OK;
}

extern "C" {

// The read-back of asmc_importance_result put on the stream NOW, with an event behind it: a caller that enqueues more work
// behind the step (the gather's consumers: asmc_mean_gram_enqueue) can then collect the step's scalars as soon as the step
// itself is done, while that work is still running.
int asmc_importance_result_enqueue(asmc_ctx* ctx, asmc_stream stream) {
    ASMC_REQUIRE(ctx != nullptr, "null ctx");
    hipStream_t st = as_stream(stream);
    const int rc = isw_readback_enqueue(ctx, st);
    if (rc) return rc;
    if (!ctx->ev_is) ASMC_HIP(hipEventCreateWithFlags(&ctx->ev_is, hipEventDisableTiming));
    ASMC_HIP(hipEventRecord(ctx->ev_is, st));
    ctx->is_result_pending = 1;
    return ASMC_OK;
}

int asmc_importance_result(asmc_ctx* ctx, double* out_host, asmc_stream stream) {
    ASMC_REQUIRE(ctx && out_host, "null pointer");
    hipStream_t st = as_stream(stream);
    double* h = ctx->h_pinned + HP_STEP_RESULT;
    unsigned int* hp = reinterpret_cast<unsigned int*>(h + ISW_OUT_LEN);
    if (ctx->is_result_pending) {  // asmc_importance_result_enqueue has put the copies on the stream already
        ctx->is_result_pending = 0;
        ASMC_HIP(hipEventSynchronize(ctx->ev_is));
    } else {
        const int rc = isw_readback_enqueue(ctx, st);
        if (rc) return rc;
        ASMC_HIP(hipStreamSynchronize(st));
    }
    bis_result(out_host, h, h[BIS_NAN]);
    out_host[13] = h[ISW_OUT_M2], out_host[14] = h[ISW_OUT_S1P], out_host[15] = h[ISW_OUT_FOUND];
    if (hp[0] != 0) {
        // a grid barrier timed out (isw_barrier): nothing of this step is valid; reset the counters and leave the
        // persistent kernel alone from now on - the caller redoes the step through the step-by-step entry points
        ASMC_HIP(hipMemsetAsync(ctx->d_bar, 0, sizeof(unsigned int) * BAR_ISW_RESET_LEN, st));
        memset(ctx->bar_base, 0, sizeof(ctx->bar_base));
        ctx->isw_disabled = 1;
        out_host[2] = 0.0, out_host[9] = 0.0, out_host[15] = 0.0;
    }
#ifdef ISW_STAMP
    fprintf(stderr, "k_is_weights stamps (us, block 0):");
    for (int k = ISW_OUT_STAMPS; k < ISW_OUT_STAMPS + 16; k++) fprintf(stderr, " %.2f", h[k]);
    fprintf(stderr, "\n");
#endif
    return ASMC_OK;
}

int asmc_importance_available(asmc_ctx* ctx) { return ctx && !ctx->isw_disabled ? 1 : 0; }

// The scan-tile sums the last asmc_importance_step's weight kernel left in the context's scratch (one per ASMC_SCAN_TILE
// particles; the exact scan behind it reads them as hints and leaves them alone while there are at most 1024 tiles), copied
// to out_dev[ceil(n / ASMC_SCAN_TILE)] on the stream: a read-back for tests and diagnostics.
int asmc_importance_tile_sums(asmc_ctx* ctx, int64_t n, double* out_dev, asmc_stream stream) {
    ASMC_REQUIRE(ctx && out_dev, "null pointer");
    ASMC_REQUIRE(n > 0 && n <= ctx->n_max, "n out of range for this ctx");
    const int64_t n_tiles = scan_tiles(n);
    ASMC_REQUIRE(n_tiles <= 1024, "above 1024 tiles the scan overwrites the tile sums with their prefix");
    ASMC_HIP(hipMemcpyAsync(out_dev, ctx->d_tiles, sizeof(double) * (size_t)n_tiles, hipMemcpyDeviceToDevice, as_stream(stream)));
    return ASMC_OK;
}

}  // extern "C"
