// asmc_scratch.h — the one map of the context's shared scratch: ctx->d_small, ctx->h_pinned, ctx->d_tiles, ctx->d_tiles_i,
// ctx->d_flags, ctx->d_bar and the tail of ctx->d_keys.
// Included by asmc_common.h behind struct asmc_ctx; no other file adds a number to one of these pointers.
//
// Every region has an offset and a length in elements of its buffer, an owner (the file whose calls write it) and a
// lifetime class:
//   TRANSIENT  written and consumed inside one exported call (the call synchronises, or its own launches read it)
//   HELD       written by an enqueue and read by a LATER call: a fetch, a result call, the next pass of a chain
// Transient regions may alias one another (the stream orders the calls).  A held region must not be touched by anything
// else while it is held; the static_asserts at the end check that for every pair, bar the overlaps listed there, which
// exist today and are documented instead of moved (moving a region changes behaviour: a change of its own).
#pragma once

// ---- ctx->d_small: doubles on the device -------------------------------------------------------------------------------
constexpr int DS_LEN = 4096;
constexpr int DS_REDUCE = 0;             // TRANSIENT  asmc_weights.hip, asmc_moments.hip: result vectors of the reduction
constexpr int DS_REDUCE_LEN = 1024;      //            kernels (k_finalize_columns, k_reduce_columns), copied out by the same call
constexpr int DS_CDF_TOTAL = 1024;       // HELD       asmc_cdf.hip: the last cdf's total (asmc_cdf, asmc_importance_step) until
                                         //            asmc_cdf_normalize_last / asmc_cdf_total_dev read it
constexpr int DS_CDF_APPROX_TOTAL = 1025;  // TRANSIENT asmc_cdf.hip: parallel-order total behind k_scan_tiles<false>
constexpr int DS_GRAM_CENTER = 2048;     // TRANSIENT  asmc_moments.hip: the Gram kernels' centre (asmc_student.hip zeroes it)
constexpr int DS_GRAM_CENTER_LEN = 128;
constexpr int DS_REF_STATUS = 2300;      // TRANSIENT  asmc_moments.hip, asmc_student.hip: k_ref_factor's status, copied to a
                                         //            pinned cell by the same call
constexpr int DS_STUDENT_EM = 2320;      // TRANSIENT  asmc_student.hip: the EM's scalars
constexpr int DS_STUDENT_EM_LEN = 8;
constexpr int DS_BISECT = 2560;          // HELD       asmc_search.hip, asmc_is_weights.hip: state record of the beta search (k_bis_sums,
constexpr int DS_BISECT_REC = 64;        //            k_is_weights) until the result call copies it out; the folded sharded
constexpr int DS_BISECT_LEN = 2 * DS_BISECT_REC;  //    search alternates between two records (round r in record r & 1)
constexpr int DS_TRTAB = 3072;           // TRANSIENT  asmc_pcn.hip: packed table of the transform epilogue (k_trtab_pack)
#define TRTAB_ROWS 14                    //            TRTAB_ROWS rows of D <= 32 doubles, then TRTAB_SCALARS scalars
#define TRTAB_SCALARS 8
constexpr int DS_TRTAB_LEN = TRTAB_ROWS * 32 + TRTAB_SCALARS;

// ---- ctx->h_pinned: doubles in pinned host memory ------------------------------------------------------------------------
constexpr int HP_LEN = 8192;
constexpr int HP_FRONT = 0;              // TRANSIENT  every file: a call's scalar read-back or small upload; the call waits for
constexpr int HP_FRONT_LEN = 128;        //            the stream before it returns (bare ctx->h_pinned is this region)
// read-back of a mutation call (asmc_pcn.hip): HELD from asmc_pcn_mutate_flow_enqueue to asmc_pcn_mutate_flow_result; the
// blocking calls fill and read the same cells inside one call
constexpr int HP_PCN_COUNTS = 0;         // HELD       accept counts, one int64 per step
constexpr int HP_PCN_COUNTS_LEN = ASMC_MAX_PCN_STEPS;
constexpr int HP_PCN_RHO_HEAD = ASMC_MAX_PCN_STEPS;  // HELD  flow calls copy d_rho = {rho, 7 unused} | history in one piece:
constexpr int HP_PCN_RHO_HEAD_LEN = 8;   //            rho lands here, the history right behind it
constexpr int HP_PCN_RHO_HIST = HP_PCN_RHO_HEAD + HP_PCN_RHO_HEAD_LEN;  // HELD  step-size history, one double per step
constexpr int HP_PCN_RHO_HIST_LEN = ASMC_MAX_PCN_STEPS;
constexpr int HP_PCN_RHO = 8000;         // HELD       the step size, where a call copies it on its own (asmc_pcn_mutate)
constexpr int HP_PCN_NONFINITE = 8001;   // HELD       non-finite flow densities among the proposals (u64)
constexpr int HP_PCN_LQ_COUNTS = 8002;   // HELD       {NaN, inf} counts of the carried log q (u64 each)
constexpr int HP_PCN_LQ_COUNTS_LEN = 2;
constexpr int HP_GRAM_CENTER = 2048;     // TRANSIENT  asmc_moments.hip: staging of asmc_centered_gram's centre
constexpr int HP_GRAM_CENTER_LEN = 128;
constexpr int HP_PCG_TAB = 4096;         // TRANSIENT  asmc_resample.hip: staging of the PCG64 jump table (u64), rebuilt when the
constexpr int HP_PCG_TAB_LEN = 256;      //            generator's increment changes
constexpr int HP_STEP_RESULT = 4096 + 512;  // HELD    asmc_is_weights.hip: the importance step's result record, from
constexpr int HP_STEP_RESULT_LEN = 40 + 4 * 64;  //    asmc_importance_result_enqueue to asmc_importance_result (search state
                                         //            [64], poison word); asmc_find_beta, asmc_find_beta_shard_result and
                                         //            asmc_shard_step_result (40 + 4 world doubles) fill and read it in one call
constexpr int REF_STATUS_CELL0 = 8010;   // HELD       asmc_moments.hip: ring of factorisation status cells, one per request,
constexpr int REF_STATUS_CELLS = 16;     //            from asmc_reference_factor to asmc_reference_factor_status(_of)

// ---- ctx->d_tiles (doubles) and ctx->d_tiles_i (int64): n_tiles_max entries per array, all TRANSIENT ---------------------------
// (the tile sums of an importance step stay readable by asmc_importance_tile_sums until the next launch that writes tiles)
constexpr size_t scratch_tiles_len(int64_t n_tiles_max) { return (size_t)(n_tiles_max * 4 + 64); }
constexpr size_t scratch_tiles_i_len(int64_t n_tiles_max) { return (size_t)(n_tiles_max * 8 + 64); }
// d_tiles: [0, T) tile sums, then their prefixes (k_tile_sum / k_is_weights, k_scan_tiles)   [2T, 3T) exact sum entering a
// tile   [3T, 4T) exact sum behind a flag-2 tile's crossing (asmc_cdf.hip)
static inline double* scratch_tile_s(const asmc_ctx* ctx) { return ctx->d_tiles + ctx->n_tiles_max * 2; }
static inline double* scratch_tile_s2(const asmc_ctx* ctx) { return ctx->d_tiles + ctx->n_tiles_max * 3; }
// d_tiles_i: [0, 4T) tile_info of the exact cdf, 4 per tile (asmc_cdf.hip) - or [0, T) per-tile counts of a compaction /
// range selection (asmc_resample.hip)   [4T, 8T) tile_split, 4 per tile   [8T] total of the counts
static inline long long* scratch_tile_split(const asmc_ctx* ctx) { return ctx->d_tiles_i + ctx->n_tiles_max * 4; }
static inline long long* scratch_count_total(const asmc_ctx* ctx) { return ctx->d_tiles_i + ctx->n_tiles_max * 8; }
constexpr bool scratch_tiles_fit(int64_t t) { return 4 * t <= (int64_t)scratch_tiles_len(t) && 8 * t + 1 <= (int64_t)scratch_tiles_i_len(t); }
static_assert(scratch_tiles_fit(1) && scratch_tiles_fit(1 << 20), "four / eight entries per tile and the total lie inside the tile arrays");

// ---- ctx->d_flags: bytes right behind the fused step's counters, inside ctx->d_tilectr's allocation; all TRANSIENT ----------------
// Three users, each inside one exported call (a context carries one mutation at a time):
//   accept flags   [0, n)             asmc_pcn.hip: the split path's accept decision (pcn_accept_flags_launch -> launch_copy_flagged)
//   tile parities  [0, ceil(n / 64))  a fused flow mutation: which half of the state holds a tile.  Zeroed by the call; the in-place
//                                     build (FUSED_INPLACE 1) never flips one, but the call's un-whitening launch READS them
//                                     (k_pcn_reg, PCN_UNWHITEN_X) - so nothing else of that call may live in these bytes
//   moved marks    [P, P + n)         P = scratch_flags_moved_off(n), behind the parities.  A fused flow mutation at beta = 1: 1 where
//                                     a step without the density accepted; zeroed by the call's fill, written by its steps, read by
//                                     its one log q refresh, dead after it
// The call's fill covers the counters in front and these bytes in one piece, rounded up to 16 bytes (a ragged memset is two fill kernels).
constexpr size_t SCRATCH_FLAGS_SLACK = 64;
constexpr size_t scratch_flags_len(int64_t n_max) { return (size_t)n_max + (size_t)n_max / 64 + SCRATCH_FLAGS_SLACK; }
constexpr size_t scratch_flags_fill(int64_t entries) { return ((size_t)entries + 15) / 16 * 16; }
constexpr size_t scratch_flags_moved_off(int64_t n) { return scratch_flags_fill((n + 63) / 64); }
constexpr bool scratch_flags_fit(int64_t n) { return scratch_flags_moved_off(n) + scratch_flags_fill(n) <= scratch_flags_len(n); }
static_assert(scratch_flags_fit(1) && scratch_flags_fit(63) && scratch_flags_fit(193) && scratch_flags_fit(1 << 20) && scratch_flags_fit((1 << 20) + 1),
              "parities and moved marks, each rounded to 16 bytes, stay inside the allocation");

// ---- ctx->d_bar: 32-bit words on the device, zeroed at creation ----------------------------------------------------------------
// The grid barrier of the persistent importance-weight kernel (asmc_is_weights.hip) and, behind its cells, three self-resetting
// counters of other kernels.  asmc_importance_result zeroes words [0, BAR_ISW_RESET_LEN) after a barrier time-out: that range must
// end in front of the cells of the other owners (checked below).
constexpr int BAR_LEN = 1024 * 17;
constexpr int ISW_GROUPS = 8;            //            arrival groups of the barrier (isw_barrier)
constexpr int ISW_BAR_STRIDE = 1024;     //            its counters lie 4 KB apart (different memory channels)
constexpr int BAR_ISW_TOP = 0;           // HELD       asmc_is_weights.hip: top counter; group g counts in word ISW_BAR_STRIDE * (1 + g).
                                         //            They only grow: held from launch to launch (ctx->bar_base[] mirrors them)
constexpr int ISW_POISON_CELL = ISW_BAR_STRIDE * (ISW_GROUPS + 2);  // HELD  asmc_is_weights.hip: raised by a barrier that timed out,
                                         //            until asmc_importance_result reads it and resets the range below
constexpr int BAR_ISW_RESET_LEN = ISW_BAR_STRIDE * (ISW_GROUPS + 3);  //  words that reset covers
constexpr int SHARD_TICKET_CELL = 1024 * 12;  // TRANSIENT  asmc_search.hip: arrival counter of k_weights_m2_lse_shard (the last
                                         //            block zeroes it again)
constexpr int COUNT_CELLS = 1024 * 12 + 64;  // HELD   asmc_weights.hip: two {NaN, inf} count slots of k_count_nonfinite (u64 each), used in
constexpr int COUNT_CELLS_LEN = 8;       //            turn, from asmc_count_nonfinite_enqueue to the read-back of asmc_count_slot
static_assert(BAR_ISW_TOP + ISW_BAR_STRIDE * (1 + ISW_GROUPS) <= ISW_POISON_CELL && ISW_POISON_CELL < BAR_ISW_RESET_LEN,
              "the barrier's counters and the poison cell lie inside the range a time-out resets");
static_assert(BAR_ISW_RESET_LEN <= SHARD_TICKET_CELL && BAR_ISW_RESET_LEN <= COUNT_CELLS,
              "the reset after a barrier time-out ends in front of the shard ticket and the count slots");
static_assert(SHARD_TICKET_CELL < COUNT_CELLS && COUNT_CELLS + COUNT_CELLS_LEN <= BAR_LEN, "every cell of d_bar lies inside its allocation");
static_assert(COUNT_CELLS % 2 == 0, "the count slots are 8-byte cells in an array of 4-byte words");
static_assert(sizeof(asmc_ctx::bar_base) / sizeof(unsigned int) >= 1 + ISW_GROUPS, "ctx->bar_base[] mirrors the top counter and every group");

// ---- ctx->d_keys: 64-bit words on the device; [0, ASMC_MAX_BETAS) atomicMax keys, one per candidate (k_weights_max), then ----------
constexpr int KEYS_LEN = ASMC_MAX_BETAS + 8;
constexpr int KEYS_NAN = ASMC_MAX_BETAS;         // HELD  asmc_weights.hip: NaN log-weights the last k_weights_max counted, until the
                                                 //       search that enqueued it has read it (k_bis_sums' record, asmc_find_beta)
constexpr int KEYS_SEARCH_TICKET = ASMC_MAX_BETAS + 4;  // HELD  asmc_search.hip: arrival counter of k_bis_sums (its low 32 bits), over
                                                 //       the rounds of one search; the max pass's memset zeroes the whole array
static_assert(KEYS_NAN < KEYS_SEARCH_TICKET && KEYS_SEARCH_TICKET < KEYS_LEN, "the key tail lies inside its allocation");

// ---- the checks ------------------------------------------------------------------------------------------------------------
struct ScratchRegion {
    int buf, off, len, held;  // buf: 0 = d_small, 1 = h_pinned
};
enum {
    R_DS_REDUCE, R_DS_CDF_TOTAL, R_DS_CDF_APPROX_TOTAL, R_DS_GRAM_CENTER, R_DS_REF_STATUS, R_DS_STUDENT_EM, R_DS_BISECT, R_DS_TRTAB,
    R_HP_FRONT, R_HP_PCN_COUNTS, R_HP_PCN_RHO_HEAD, R_HP_PCN_RHO_HIST, R_HP_PCN_RHO, R_HP_PCN_NONFINITE, R_HP_PCN_LQ_COUNTS,
    R_HP_GRAM_CENTER, R_HP_PCG_TAB, R_HP_STEP_RESULT, R_HP_REF_STATUS, R_COUNT
};
constexpr ScratchRegion SCRATCH_MAP[R_COUNT] = {
    {0, DS_REDUCE, DS_REDUCE_LEN, 0},
    {0, DS_CDF_TOTAL, 1, 1},
    {0, DS_CDF_APPROX_TOTAL, 1, 0},
    {0, DS_GRAM_CENTER, DS_GRAM_CENTER_LEN, 0},
    {0, DS_REF_STATUS, 1, 0},
    {0, DS_STUDENT_EM, DS_STUDENT_EM_LEN, 0},
    {0, DS_BISECT, DS_BISECT_LEN, 1},
    {0, DS_TRTAB, DS_TRTAB_LEN, 0},
    {1, HP_FRONT, HP_FRONT_LEN, 0},
    {1, HP_PCN_COUNTS, HP_PCN_COUNTS_LEN, 1},
    {1, HP_PCN_RHO_HEAD, HP_PCN_RHO_HEAD_LEN, 1},
    {1, HP_PCN_RHO_HIST, HP_PCN_RHO_HIST_LEN, 1},
    {1, HP_PCN_RHO, 1, 1},
    {1, HP_PCN_NONFINITE, 1, 1},
    {1, HP_PCN_LQ_COUNTS, HP_PCN_LQ_COUNTS_LEN, 1},
    {1, HP_GRAM_CENTER, HP_GRAM_CENTER_LEN, 0},
    {1, HP_PCG_TAB, HP_PCG_TAB_LEN, 0},
    {1, HP_STEP_RESULT, HP_STEP_RESULT_LEN, 1},
    {1, REF_STATUS_CELL0, REF_STATUS_CELLS, 1},
};
// Overlaps of a held region with a transient one that exist at today's offsets.  All three are in h_pinned and all three have
// the read-back of a DEFERRED mutation as their held side (asmc_pcn_mutate_flow_enqueue ... asmc_pcn_mutate_flow_result); a
// blocking mutation call is not affected.  The one caller that defers (the SMC sampler's look-ahead) puts asmc_importance_step,
// asmc_gather, asmc_importance_result_enqueue, asmc_mean_gram_enqueue and asmc_reference_factor in between, none of which
// writes one of these transient regions - except the jump-table staging, which that caller keeps clear of by deferring at most
// 1024 steps.  A caller of the C interface can hit each of them:
//   HP_FRONT x HP_PCN_COUNTS        enqueue; any call that reads a scalar back through the front (asmc_cdf with total_host,
//                                   asmc_select_range, asmc_compact_valid, asmc_weights_m2, asmc_count_nonfinite, ...); result:
//                                   the counts of the first steps are that call's scalars
//   HP_GRAM_CENTER x HP_PCN_RHO_HEAD, HP_PCN_RHO_HIST
//                                   enqueue; asmc_centered_gram (its memcpy of the centre is not even stream-ordered); result:
//                                   rho and the first step sizes are the centre, or the mutation's copy lands in a centre
//                                   that is still being uploaded
//   HP_PCG_TAB x HP_PCN_RHO_HIST    enqueue with n_steps > SCRATCH_HIST_SAFE_STEPS; a call with a generator of another increment
//                                   (asmc_importance_step, asmc_pcg64_uniforms, asmc_pcg64_select); result: the step sizes
//                                   of the last steps are jump-table words
constexpr int SCRATCH_KNOWN_OVERLAPS[][2] = {
    {R_HP_PCN_COUNTS, R_HP_FRONT},
    {R_HP_PCN_RHO_HEAD, R_HP_GRAM_CENTER},
    {R_HP_PCN_RHO_HIST, R_HP_GRAM_CENTER},
    {R_HP_PCN_RHO_HIST, R_HP_PCG_TAB},
};
constexpr int SCRATCH_HIST_SAFE_STEPS = HP_PCG_TAB - HP_PCN_RHO_HIST;  // 2040 of ASMC_MAX_PCN_STEPS = 2048

constexpr bool scratch_overlap(const ScratchRegion& a, const ScratchRegion& b) {
    return a.buf == b.buf && a.off < b.off + b.len && b.off < a.off + a.len;
}
constexpr bool scratch_known_overlap(int i, int j) {
    for (const auto& k : SCRATCH_KNOWN_OVERLAPS)
        if ((k[0] == i && k[1] == j) || (k[0] == j && k[1] == i)) return true;
    return false;
}
// first region that leaves its buffer, or -1
constexpr int scratch_first_outside() {
    for (int i = 0; i < R_COUNT; i++)
        if (SCRATCH_MAP[i].off < 0 || SCRATCH_MAP[i].len < 1 || SCRATCH_MAP[i].off + SCRATCH_MAP[i].len > (SCRATCH_MAP[i].buf ? HP_LEN : DS_LEN))
            return i;
    return -1;
}
// first held region that overlaps another region (held or transient) outside the list above, or -1
constexpr int scratch_first_clash() {
    for (int i = 0; i < R_COUNT; i++)
        for (int j = 0; j < R_COUNT; j++)
            if (i != j && SCRATCH_MAP[i].held && scratch_overlap(SCRATCH_MAP[i], SCRATCH_MAP[j]) && !scratch_known_overlap(i, j)) return i;
    return -1;
}
// a listed overlap that no longer exists must leave the list
constexpr bool scratch_known_overlaps_real() {
    for (const auto& k : SCRATCH_KNOWN_OVERLAPS)
        if (!scratch_overlap(SCRATCH_MAP[k[0]], SCRATCH_MAP[k[1]]) || !SCRATCH_MAP[k[0]].held || SCRATCH_MAP[k[1]].held) return false;
    return true;
}
static_assert(scratch_first_outside() == -1, "a scratch region leaves its buffer");
static_assert(scratch_first_clash() == -1, "a held scratch region overlaps another region");
static_assert(scratch_known_overlaps_real(), "SCRATCH_KNOWN_OVERLAPS lists held x transient overlaps that exist, nothing else");
// the weakened form of `step-size history x jump-table staging`: disjoint up to SCRATCH_HIST_SAFE_STEPS steps per call
static_assert(SCRATCH_HIST_SAFE_STEPS == 2040 && HP_PCN_RHO_HIST + SCRATCH_HIST_SAFE_STEPS <= HP_PCG_TAB, "history x jump-table staging");
static_assert(HP_PCN_RHO_HIST + HP_PCN_RHO_HIST_LEN <= HP_STEP_RESULT, "the longest history stays in front of the result record");
