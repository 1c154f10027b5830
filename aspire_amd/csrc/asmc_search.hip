// asmc_search.hip — the adaptive-temperature search on the device (smc/base.py:167-186): k_bis_sums, one search round per launch,
// and k_bis_decide, the decide half of a sharded round; asmc_find_beta and the asmc_find_beta_shard_* calls.
// Behind them the weight passes of the one-chain sharded importance step, which read the search's state on the device:
// k_weights_m2_lse_shard (it also closes the last round of a folded search: bis_shard_decide, as k_bis_sums does for the
// rounds before) and k_weights_map_shard, with asmc_weights_m2_lse_shard, asmc_normalized_weights_shard, asmc_shard_step_result.
// The round tail, the state record's helpers and the merge of rank records: asmc_search_dev.h; the decisions: asmc_bisect.h.
// The maximum pass in front of a search is asmc_weights.hip's (asmc_weights_max_launch).
#include "asmc_search_dev.h"

// One bisection round in ONE launch.  The 15 candidates and the bracket's upper end are equally spaced,
// beta_j = beta_1 + (j-1) h (j = 1..16), and every log-sum-exp is shifted by m_j = (beta_j - beta0) Delta_max, so for
// particle i
//     exp(lw_i(beta_j) - m_j) = exp(lw_i(beta_1) - m_1) * r_i^(j-1),   r_i = exp(h (Delta_i - Delta_max)) <= 1:
// two exponentials per particle instead of sixteen.  The first factor uses the reference's own expression for the
// log-weight (samples.py:1222-1224); the progression is non-increasing in j, so it can neither overflow nor lose
// a term that matters.  Deviation from the long-double sums of the exact log-weights at the node's float, per term and
// relative (u = 2^-53; DESIGN.md section 3.16, tests/weights_ref.py): u (8 t (|lq| + |ll + lp|) + |lw| + 4 |lw - m|) + 6 u |m|
// + (LU + 1) u (|Delta - Delta_max| + |Delta_max|) + (15 + L) u + 2 E, t = beta - beta0, LU the depth of the dyadic grid, L the
// addition chain, E = 3.4 u the bound on exp.  That is 1e-14 .. 1e-13 for |Delta|, |lq| of order 10 .. 100 and grows in
// proportion: 1e-10 at |Delta| = 3e4, 1e-9 with a common offset of 1e6 in ll and lq (where the reference's own fp64 expression
// has lost as much).  Measured: below 0.3 of that bound on every population of tests/test_gpu_weights.py.  It decides
// `eff >= target` comparisons; the values reported at the chosen beta carry the same bound.
// The block that arrives last (ticket counter behind an agent-scope release) reduces the partials and runs the
// tail, so a round costs one launch; the first round derives its grid from m(1) (max kernel) itself.
#define BIS_THREADS 512  // one block per CU: few, large partial records keep the last block's reduction short

__global__ __launch_bounds__(BIS_THREADS) void k_bis_sums(int64_t n, const double* __restrict__ ll,
                                                        const double* __restrict__ lp, const double* __restrict__ lq,
                                                        double* __restrict__ st,
                                                        double* partials, unsigned int* ticket, int round, BisInit init,
                                                        const unsigned long long* __restrict__ keys,
                                                        double* __restrict__ rec_out,
                                                        const double* __restrict__ recs_prev = nullptr, int world = 0,
                                                        const double* __restrict__ st_prev = nullptr) {
    __shared__ double s_red[BIS_THREADS / 32][33];
    __shared__ double s_S[32];
    __shared__ double s_eff[16];
    __shared__ BisLds Lf;  // folded sharded rounds (recs_prev given): the state after the previous round's decide half
    BisGrid g;
    double m_one = 0.0, m_base = 0.0;
    if (recs_prev) {
        // round >= 1 of the one-chain sharded step: the previous round is closed HERE, by every block, from the gathered
        // records; block 0 leaves the state in `st` (the other of the two state buffers: nobody reads what is being written)
        bis_shard_decide(Lf, recs_prev, world, round - 1, init, st_prev, s_S, s_eff);
        if (blockIdx.x == 0 && threadIdx.x < BIS_STATE_LEN) st[threadIdx.x] = Lf.st[threadIdx.x];
        if (Lf.st[BIS_DONE] != 0.0) return;
        g = bis_next_grid(Lf.st), m_base = Lf.st[BIS_M_ONE];
        __syncthreads();  // (s_S, s_eff are reused by the last block below)
    } else if (round == 0) {
        m_one = key_to_f64(keys[0]);
        // sharded search: a rank without a finite log-weight (local m(1) = -inf) reduces against 0, as a block of k_is_weights
        // does - its sums are then zero, not exp(-inf + inf) = NaN, and the merge of the rank records (k_bis_decide,
        // bis_shard_decide) gives them the factor exp(-inf) = 0 against the other ranks' maximum.  The record still reports
        // -inf.  The single-rank search keeps the reference's NaN for a population without any finite log-weight.
        g = bis_first_grid(init.beta0, (rec_out && m_one == -INFINITY) ? 0.0 : m_one);
    } else {
        if (st[BIS_DONE] != 0.0) return;  // converged in an earlier round (uniform across the grid)
        g = bis_next_grid(st);
    }
    double s1[16], s2[16];
#pragma unroll
    for (int j = 0; j < 16; j++) s1[j] = 0.0, s2[j] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * BIS_THREADS;
    // two particles per trip: six loads in flight before the first exponential
    for (int64_t i = (int64_t)blockIdx.x * BIS_THREADS + threadIdx.x; i < n; i += 2 * stride) {
        const int64_t i2 = i + stride;
        const bool has2 = i2 < n;
        const double a = ll[i], b = lp[i], q = lq[i];
        const double a2 = has2 ? ll[i2] : 0.0, b2 = has2 ? lp[i2] : 0.0, q2 = has2 ? lq[i2] : 0.0;
        const double e = exp(lw_of(a, b, q, g.c1, g.c2) - g.m1);
        const double r = exp(g.h * (((a + b) - q) - g.dmax));
        const double e2 = has2 ? exp(lw_of(a2, b2, q2, g.c1, g.c2) - g.m1) : 0.0;
        const double r2 = has2 ? exp(g.h * (((a2 + b2) - q2) - g.dmax)) : 0.0;
        bis_accumulate(s1, s2, e, r, e2, r2);
    }
    __shared__ double s_p[BIS_THREADS / 64][32];
    bis_block_record<BIS_THREADS / 64>(s1, s2, s_p, partials);
    // The block that arrives last closes the round.  The counter is zeroed once per search by a memset on the stream and
    // only ever grows: round r ends at ticket (r+1) * grid - 1.
    if (!bis_last_block(ticket, (unsigned int)(round + 1) * gridDim.x - 1u, false)) return;
    if (rec_out) {
        // sharded search: this rank's column sums, the shift base they are relative to (local m(1) in the first
        // round, the merged one afterwards) and the local NaN census leave as one record; k_bis_decide closes the round
        // on every rank after the all-gather
        bis_reduce_partials(partials, (int)gridDim.x, s_red, s_S);
        __syncthreads();
        if (threadIdx.x < 32) rec_out[threadIdx.x] = s_S[threadIdx.x];
        if (threadIdx.x == 32) rec_out[32] = round == 0 ? m_one : recs_prev ? m_base : st[BIS_M_ONE];
        if (threadIdx.x == 33) rec_out[33] = round == 0 ? (double)keys[KEYS_NAN] : 0.0;
        return;
    }
    bis_tail_body(st, partials, (int)gridDim.x, round == 0, m_one, init, s_red, s_S, s_eff);
}

// Sharded search, second half of a round (every rank runs it on the same all-gathered records, so every rank takes
// the same decisions): load the state, merge the rank records (bis_merge_records), run the tail of the single-rank kernel.
__global__ __launch_bounds__(BIS_THREADS) void k_bis_decide(const double* __restrict__ recs, int world,
                                                          double* __restrict__ st, int round, BisInit init) {
    __shared__ double s_red[BIS_THREADS / 32][33];
    __shared__ double s_S[32];
    __shared__ double s_eff[16];
    if (round > 0 && st[BIS_DONE] != 0.0) return;  // converged earlier
    double nan_total;
    const double m_all = bis_merge_records(recs, world, round, init.beta0, s_S, nan_total);
    __syncthreads();
    bis_tail_body(st, nullptr, 0, round == 0, m_all, init, s_red, s_S, s_eff, nan_total);
}

// Sharded importance step: k_weights_m2_lse and k_weights_map<1> with their scalars taken from the search state the last k_bis_decide left
// on the device (st[BIS_*], identical on every rank) - no host decision sits between the search, the evidence moments and
// the weights.  The scalars are formed in smc_math.resample_owner's operation order (= k_is_weights' phase 2).
struct ShardScalars {
    double c1, c2, m, mean_u, shift, mp;
    bool found;
};
__device__ __forceinline__ ShardScalars shard_scalars(const double* __restrict__ st) {
    ShardScalars s;
    const double beta0 = st[BIS_BETA0], beta = st[BIS_BMIN], N = st[BIS_N];
    s.found = st[BIS_DONE] != 0.0 && st[BIS_TRIP_OK] != 0.0 && st[BIS_NAN] == 0.0 && beta > beta0;
    s.c1 = beta0 - beta, s.c2 = beta - beta0;
    s.m = st[BIS_TRIP_M];
    const double S1 = st[BIS_TRIP_S1];
    s.mean_u = S1 / N;
    s.shift = (s.m + log(S1)) - st[BIS_LOGN];
    s.mp = s.m + s.shift;
    return s;
}

__global__ __launch_bounds__(ASMC_BLOCK) void k_weights_m2_lse_shard(int64_t n, const double* __restrict__ ll,
                                                                    const double* __restrict__ lp,
                                                                    const double* __restrict__ lq,
                                                                    const double* __restrict__ st,
                                                                    double* partials, unsigned int* ticket,
                                                                    double* __restrict__ out,
                                                                    const double* __restrict__ recs_last, int world,
                                                                    int last_round, BisInit init, double* __restrict__ st_out) {
    __shared__ BisLds Lf;
    __shared__ double s_S[32];
    __shared__ double s_eff[16];
    if (recs_last) {  // the search's last round is closed here (bis_shard_decide); block 0 leaves the final state in st_out
        bis_shard_decide(Lf, recs_last, world, last_round, init, st, s_S, s_eff);
        if (blockIdx.x == 0 && threadIdx.x < BIS_STATE_LEN) st_out[threadIdx.x] = Lf.st[threadIdx.x];
    }
    const ShardScalars s = shard_scalars(recs_last ? Lf.st : st);
    m2_lse_block(n, ll, lp, lq, s.c1, s.c2, s.m, s.mean_u, s.shift, s.mp, s.found, partials);
    // k_finalize_columns by the block that arrives last (the counter resets itself for the next call)
    if (!bis_last_block(ticket, gridDim.x - 1u, true) || threadIdx.x >= 128) return;
    {
        const int col = threadIdx.x >> 6, lane = threadIdx.x & 63;
        double v = 0.0;
        for (int b = lane; b < (int)gridDim.x; b += 64) v += __builtin_nontemporal_load(partials + (size_t)b * 2 + col);
        v = wave_sum(v);
        if (lane == 0) out[col] = v;
    }
}

// w = exp((lw + shift) - lse) with lse = mp + log(S1'), S1' = the ranks' second sums added in rank order (parts[world][2], the
// all-gathered outputs of the pass above); carry_out[0] = this rank's approximate incoming cdf sum (the lower ranks' share).
// A search that has not converged (or NaN weights, or an empty sum) leaves uniform weights and the uniform carry: everything
// enqueued behind stays well defined, the host discards it when it reads the state.
__global__ __launch_bounds__(ASMC_BLOCK) void k_weights_map_shard(int64_t n, const double* __restrict__ ll,
                                                                 const double* __restrict__ lp,
                                                                 const double* __restrict__ lq,
                                                                 const double* __restrict__ st,
                                                                 const double* __restrict__ parts, int world, int rank,
                                                                 double carry_uniform, double* __restrict__ out,
                                                                 double* __restrict__ carry_out,
                                                                 double* __restrict__ tile_sums,
                                                                 double* __restrict__ st_copy, double* __restrict__ rec) {
    const ShardScalars s = shard_scalars(st);
    double s1p = parts[1], below = 0.0;
    for (int r = 1; r < world; r++) {
        if (r == rank) below = s1p;
        s1p += parts[2 * r + 1];
    }
    const bool found = s.found && s1p > 0.0 && s1p < INFINITY;
    const double lse = s.mp + log(s1p);
    const double w_uniform = 1.0 / st[BIS_N];
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) carry_out[0] = found ? below / s1p : carry_uniform;
        if (st_copy && threadIdx.x < BIS_STATE_LEN) st_copy[threadIdx.x] = st[threadIdx.x];  // the search state, next to parts / info
    }
    // one block per scan tile (ASMC_SCAN_TILE particles): the tile's weight sum - the cdf's approximate prefix hints, any
    // order will do - leaves with the weights
    const int64_t base = (int64_t)blockIdx.x * ASMC_SCAN_TILE;
    double acc = 0.0;
#pragma unroll 4
    for (int k = 0; k < ASMC_SCAN_TILE / ASMC_BLOCK; k++) {
        const int64_t i = base + k * ASMC_BLOCK + threadIdx.x;
        if (i < n) {
            const double a = ll[i], b = lp[i], q = lq[i];
            // the (ll, lp, lq, 0) record asmc_gather reads per draw (k_pack_records' job, done on the way: asmc_rec_claim)
            if (rec) *reinterpret_cast<double4*>(rec + 4 * i) = make_double4(a, b, q, 0.0);
            const double lw = lw_of(a, b, q, s.c1, s.c2) + s.shift;
            const double wv = found ? exp(lw - lse) : w_uniform;
            out[i] = wv;
            acc += wv;
        }
    }
    __shared__ double s_t[ASMC_BLOCK / 64];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) s_t[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double v = s_t[0];
        for (int w = 1; w < ASMC_BLOCK / 64; w++) v += s_t[w];
        tile_sums[blockIdx.x] = v;
    }
}

extern "C" {

int asmc_find_beta(asmc_ctx* ctx, int64_t n, const double* ll, const double* lp, const double* lq, double beta0,
                   double target_eff, double tol, double* out_host, asmc_stream stream) {
    int rc = check_common(ctx, n, ll, lp, lq);
    if (rc) return rc;
    ASMC_REQUIRE(out_host != nullptr, "null host pointer");
    ASMC_REQUIRE(tol > 0.0 && beta0 >= 0.0 && beta0 < 1.0, "bad beta0 / tolerance");
    hipStream_t st = as_stream(stream);
    double* d_st;
    unsigned int* d_ticket;
    bis_state(ctx, &d_st, &d_ticket);
    double* h = ctx->h_pinned + HP_STEP_RESULT;
    const BisInit init = bis_init(beta0, target_eff, tol, n);
    // exact maximum at beta = 1 (also the NaN census: for beta > beta0 the NaN pattern of the log-weights does not
    // depend on beta); every round, the first one included (it evaluates beta = 1 as its 16th candidate), is then ONE launch
    const double one = 1.0;
    rc = asmc_weights_max_launch(ctx, n, ll, lp, lq, beta0, &one, 1, st);
    if (rc) return rc;
    const int grid = grid_for(n, BIS_THREADS, ctx->num_cu);
    // a plain round narrows the bracket 16x, a prediction window that holds the root by much more (asmc_bisect.h): smooth
    // populations need 3 rounds whatever the tolerance.  Three are enqueued (fewer when plain rounds reach the tolerance
    // sooner); a search that is not done after them gets further rounds one at a time.
    int rounds = (int)ceil(log2((1.0 - beta0) / tol) / BIS_LEVELS - 1e-9);
    if (rounds < 1) rounds = 1;
    if (rounds > 3) rounds = 3;
    unsigned long long* hk = reinterpret_cast<unsigned long long*>(h + BIS_STATE_LEN);
    int launched = 0;
    for (int attempt = 0; attempt < 32; attempt++) {
        for (; launched < rounds; launched++) {
            ASMC_LAUNCH(ctx, st, "k_bis_sums", k_bis_sums, dim3(grid), dim3(BIS_THREADS), 0, st, n, ll, lp, lq, d_st, ctx->d_partials,
                        d_ticket, launched, init, (const unsigned long long*)ctx->d_keys, (double*)nullptr);
            ASMC_LAUNCH_CHECK();
        }
        ASMC_HIP(hipMemcpyAsync(h, d_st, sizeof(double) * BIS_STATE_LEN, hipMemcpyDeviceToHost, st));
        ASMC_HIP(hipMemcpyAsync(hk, ctx->d_keys + KEYS_NAN, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        ASMC_HIP(hipStreamSynchronize(st));
        if (h[BIS_DONE] != 0.0) break;  // converged
        rounds++;
    }
    bis_result(out_host, h, (double)hk[0]);  // (the census of the max pass: the single-rank search keeps none in its record)
    return ASMC_OK;
}

int asmc_find_beta_shard_reduce(asmc_ctx* ctx, int64_t n, const double* ll, const double* lp, const double* lq,
                                double beta0, int round, double* rec_dev, asmc_stream stream) {
    int rc = check_common(ctx, n, ll, lp, lq);
    if (rc) return rc;
    ASMC_REQUIRE(rec_dev != nullptr && round >= 0, "null record / negative round");
    ASMC_REQUIRE(beta0 >= 0.0 && beta0 < 1.0, "bad beta0");
    hipStream_t st = as_stream(stream);
    double* d_st;
    unsigned int* d_ticket;
    bis_state(ctx, &d_st, &d_ticket);
    if (round == 0) {
        const double one = 1.0;
        rc = asmc_weights_max_launch(ctx, n, ll, lp, lq, beta0, &one, 1, st);  // local m(1), local NaN census, ticket := 0
        if (rc) return rc;
    }
    const BisInit init = {beta0, 0.0, 0.0, 0.0, 0.0, 0.0};  // the reduction half only needs beta0
    const int grid = grid_for(n, BIS_THREADS, ctx->num_cu);
    ASMC_LAUNCH(ctx, st, "k_bis_sums", k_bis_sums, dim3(grid), dim3(BIS_THREADS), 0, st, n, ll, lp, lq, d_st, ctx->d_partials,
                d_ticket, round, init, (const unsigned long long*)ctx->d_keys, rec_dev);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int asmc_find_beta_shard_decide(asmc_ctx* ctx, const double* recs_dev, int world, int64_t n_global, double beta0,
                                double target_eff, double tol, int round, asmc_stream stream) {
    ASMC_REQUIRE(ctx && recs_dev, "null pointer");
    ASMC_REQUIRE(world >= 1 && n_global > 0 && round >= 0, "bad world / n_global / round");
    ASMC_REQUIRE(tol > 0.0 && beta0 >= 0.0 && beta0 < 1.0, "bad beta0 / tolerance");
    hipStream_t st = as_stream(stream);
    double* d_st;
    unsigned int* d_ticket;
    bis_state(ctx, &d_st, &d_ticket);
    const BisInit init = bis_init(beta0, target_eff, tol, n_global);
    ASMC_LAUNCH(ctx, st, "k_bis_decide", k_bis_decide, dim3(1), dim3(BIS_THREADS), 0, st, recs_dev, world, d_st, round, init);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

// Rounds first .. last-1 of the sharded search as ONE call: reduce -> ncclAllGather of the ranks' records on the library's
// own communicator (asmc_set_rccl + asmc_set_rccl_allgather; same stream, no stream hop, no host callback) -> decide.
int asmc_find_beta_shard_rounds(asmc_ctx* ctx, int64_t n, const double* ll, const double* lp, const double* lq, double beta0,
                                double target_eff, double tol, int world, int64_t n_global, double* rec_dev, double* recs_dev,
                                int first, int last, asmc_stream stream) {
    ASMC_REQUIRE(ctx && rec_dev && recs_dev, "null pointer");
    ASMC_REQUIRE(ctx->rccl_allgather && ctx->rccl_comm, "asmc_set_rccl / asmc_set_rccl_allgather first");
    ASMC_REQUIRE(first >= 0 && last >= first, "bad round range");
    typedef int (*allgather_fn)(const void*, void*, size_t, int, void*, hipStream_t);
    const allgather_fn allgather = reinterpret_cast<allgather_fn>(ctx->rccl_allgather);
    const int nccl_f64 = 8;  // rccl.h: ncclFloat64
    for (int r = first; r < last; r++) {
        int rc = asmc_find_beta_shard_reduce(ctx, n, ll, lp, lq, beta0, r, rec_dev, stream);
        if (rc) return rc;
        if (allgather(rec_dev, recs_dev, (size_t)ASMC_BIS_REC, nccl_f64, ctx->rccl_comm, as_stream(stream)) != 0) {
            asmc_set_error("asmc_find_beta_shard_rounds: ncclAllGather failed");
            return ASMC_ERR_ARG;
        }
        rc = asmc_find_beta_shard_decide(ctx, recs_dev, world, n_global, beta0, target_eff, tol, r, stream);
        if (rc) return rc;
    }
    return ASMC_OK;
}

int asmc_find_beta_shard_result(asmc_ctx* ctx, double* out_host, asmc_stream stream) {
    ASMC_REQUIRE(ctx && out_host, "null pointer");
    hipStream_t st = as_stream(stream);
    double* h = ctx->h_pinned + HP_STEP_RESULT;
    ASMC_HIP(hipMemcpyAsync(h, ctx->d_small + DS_BISECT, sizeof(double) * BIS_STATE_LEN, hipMemcpyDeviceToHost, st));
    ASMC_HIP(hipStreamSynchronize(st));
    bis_result(out_host, h, h[BIS_NAN]);
    return ASMC_OK;
}

int asmc_find_beta_shard_round(asmc_ctx* ctx, int64_t n, const double* ll, const double* lp, const double* lq, double beta0,
                               double target_eff, double tol, int world, int64_t n_global, int round, const double* recs_prev_dev,
                               double* rec_dev, asmc_stream stream) {
    int rc = check_common(ctx, n, ll, lp, lq);
    if (rc) return rc;
    ASMC_REQUIRE(rec_dev != nullptr && round >= 0 && (round == 0 || recs_prev_dev), "null record / negative round");
    ASMC_REQUIRE(world >= 1 && n_global > 0 && tol > 0.0 && beta0 >= 0.0 && beta0 < 1.0, "bad world / n_global / beta0 / tolerance");
    if (round == 0) return asmc_find_beta_shard_reduce(ctx, n, ll, lp, lq, beta0, 0, rec_dev, stream);
    hipStream_t st = as_stream(stream);
    double* d_st;
    unsigned int* d_ticket;
    bis_state(ctx, &d_st, &d_ticket);
    const BisInit init = bis_init(beta0, target_eff, tol, n_global);
    const int grid = grid_for(n, BIS_THREADS, ctx->num_cu);
    ASMC_LAUNCH(ctx, st, "k_bis_sums", k_bis_sums, dim3(grid), dim3(BIS_THREADS), 0, st, n, ll, lp, lq, shard_state_buf(ctx, round),
                ctx->d_partials, d_ticket, round, init, (const unsigned long long*)ctx->d_keys, rec_dev, recs_prev_dev, world,
                (const double*)shard_state_buf(ctx, round - 1));
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

// Sharded importance step with device-resident scalars (include/asmc.h): the search state stays on the device, these passes
// read it there.  recs_last_dev given: the search ran as asmc_find_beta_shard_round x n_rounds and its last round is closed
// inside this pass; NULL: the state asmc_find_beta_shard_decide left.
int asmc_weights_m2_lse_shard(asmc_ctx* ctx, int64_t n, const double* ll, const double* lp, const double* lq, double* out_dev,
                              const double* recs_last_dev, int world, int64_t n_global, double beta0, double target_eff,
                              double tol, int n_rounds, asmc_stream stream) {
    int rc = check_common(ctx, n, ll, lp, lq);
    if (rc) return rc;
    ASMC_REQUIRE(out_dev != nullptr, "null device pointer");
    ASMC_REQUIRE(!recs_last_dev || (world >= 1 && n_global > 0 && n_rounds >= 1 && tol > 0.0 && beta0 >= 0.0 && beta0 < 1.0),
                 "bad world / n_global / rounds / beta0 / tolerance");
    hipStream_t st = as_stream(stream);
    double* d_st;
    unsigned int* d_ticket;
    bis_state(ctx, &d_st, &d_ticket);
    const int grid = reduce_grid(ctx, n, 1);
    BisInit init = {beta0, target_eff, tol, 0.0, 0.0, bis_plain_mode()};  // (no records to close: the kernel reads none of it)
    const double* st_in = d_st;
    double* st_out = nullptr;
    if (recs_last_dev) {
        init = bis_init(beta0, target_eff, tol, n_global);
        st_in = shard_state_buf(ctx, n_rounds - 1);
        st_out = shard_state_buf(ctx, n_rounds);
    }
    ctx->shard_st = recs_last_dev ? st_out : d_st;
    ASMC_LAUNCH(ctx, st, "k_weights_m2_lse_shard", k_weights_m2_lse_shard, dim3(grid), dim3(ASMC_BLOCK), 0, st, n, ll, lp, lq, st_in,
                ctx->d_partials, ctx->d_bar + SHARD_TICKET_CELL, out_dev, recs_last_dev, world, n_rounds - 1, init, st_out);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int asmc_normalized_weights_shard(asmc_ctx* ctx, int64_t n, const double* ll, const double* lp, const double* lq,
                                  const double* parts_dev, int world, int rank, double carry_uniform, double* w_out,
                                  double* carry_out_dev, double* tile_sums_dev, double* state_copy_dev, int pack_records,
                                  asmc_stream stream) {
    int rc = check_common(ctx, n, ll, lp, lq);
    if (rc) return rc;
    ASMC_REQUIRE(parts_dev && w_out && carry_out_dev && tile_sums_dev, "null pointer");
    ASMC_REQUIRE(world >= 1 && rank >= 0 && rank < world, "bad rank / world");
    ASMC_REQUIRE(carry_uniform >= 0.0 && carry_uniform < 1.0, "bad uniform carry");
    ASMC_REQUIRE(ctx->shard_st != nullptr, "asmc_weights_m2_lse_shard first");
    hipStream_t st = as_stream(stream);
    const int64_t n_tiles = scan_tiles(n);
    ASMC_LAUNCH(ctx, st, "k_weights_map_shard", k_weights_map_shard, dim3((unsigned)n_tiles), dim3(ASMC_BLOCK), 0, st, n, ll, lp, lq,
                (const double*)ctx->shard_st, parts_dev, world, rank, carry_uniform, w_out, carry_out_dev, tile_sums_dev, state_copy_dev,
                pack_records ? ctx->d_rec : (double*)nullptr);
    ASMC_LAUNCH_CHECK();
    if (pack_records) {  // d_rec rewritten: a new generation, held for asmc_rec_claim
        ctx->rec_token++;
        ctx->rec_hold_src[0] = ll, ctx->rec_hold_src[1] = lp, ctx->rec_hold_src[2] = lq;
        ctx->rec_hold_n = n, ctx->rec_hold_token = ctx->rec_token;
    }
    return ASMC_OK;
}

// The one synchronisation of the sharded importance step: res_dev = {search state [40] (asmc_normalized_weights_shard's
// state_copy_dev), the ranks' (m2, S1') pairs [2 world], their (kept, fail) int64 pairs [2 world]}, one contiguous buffer ->
// out_host[13 + 4 world] (asmc_find_beta_shard_result's 13 values, the pairs, the int64 pairs as doubles).
int asmc_shard_step_result(asmc_ctx* ctx, const double* res_dev, int world, double* out_host, asmc_stream stream) {
    ASMC_REQUIRE(ctx && res_dev && out_host, "null pointer");
    ASMC_REQUIRE(world >= 1 && world <= 64, "world out of range");
    hipStream_t st = as_stream(stream);
    double* h = ctx->h_pinned + HP_STEP_RESULT;
    ASMC_HIP(hipMemcpyAsync(h, res_dev, sizeof(double) * (BIS_STATE_LEN + 4 * world), hipMemcpyDeviceToHost, st));
    ASMC_HIP(hipStreamSynchronize(st));
    bis_result(out_host, h, h[BIS_NAN]);
    for (int i = 0; i < 2 * world; i++) out_host[13 + i] = h[BIS_STATE_LEN + i];
    const int64_t* hi = reinterpret_cast<const int64_t*>(h + BIS_STATE_LEN + 2 * world);
    for (int i = 0; i < 2 * world; i++) out_host[13 + 2 * world + i] = (double)hi[i];
    return ASMC_OK;
}

}  // extern "C"
