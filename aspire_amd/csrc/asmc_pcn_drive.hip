// asmc_pcn_drive.hip — the host drivers of every pCN mutation entry point: asmc_pcn_mutate, asmc_pcn_propose / _accept / _split_*,
// the asmc_pcn_ysplit_* session, asmc_pcn_mutate_flow / _enqueue / _result, and the count-hook and RCCL setters.
// No kernel lives here.  The step kernels are reached through host launch functions: asmc_pcn_shared.h (the register-resident and
// generic kernels of asmc_pcn.hip) and asmc_pcn_dev.h (matrix-core: asmc_pcn_mm.hip, fused: asmc_pcn_fused.hip, 16-particle groups:
// asmc_flow16.hip), so an edit here recompiles none of their instantiations.
//
// One copy of each sequence the entry points share: the argument check (pcn_check_call), the step scaffold (pcn_steps) and the
// call tail (pcn_finish_call).
#include <stdlib.h>

#include <chrono>

#include "asmc_pcn_shared.h"

// A call's parameters as the kernels take them: the reference, the tempering and the noise keys.  The densities and the noise
// mode are the caller's to add - a flow mutation carries a placeholder for log q, a split session no density at all.
// Everything else starts at zero (mode: PCN_X_STEP).
static PcnDev pcn_dev_from_params(const asmc_ctx* ctx, const asmc_pcn_params* prm, int d_noise) {
    PcnDev pd;
    memset(&pd, 0, sizeof(pd));
    pd.bmtab = ctx->d_bmtab;
    pd.d = prm->d;
    pd.d_noise = d_noise;
    pd.beta = prm->beta;
    pd.mu = prm->mu_dev;
    pd.L = prm->L_dev;
    pd.Linv = prm->Linv_dev;
    pd.seed = prm->seed;
    pd.gid0 = prm->gid0;
    pd.nu = prm->nu;
    return pd;
}

// ==== what the mutation entry points share ==================================================================================
// What the path that serves a call requires beyond the common arguments.
struct PcnNeeds {
    int n_mix;                  // density tables checked: 3 (ll, lp, lq) or 2 (ll, lp: the proposal density is a flow)
    bool noise;                 // the path reads prm->noise
    const asmc_coupling* flow;  // flow mutation (else NULL): flow->dims is the call's d
    bool work;                  // the call documents a work buffer of asmc_pcn_flow_work_bytes
    const void* work_dev;
    int64_t work_bytes;
};

// The argument check of asmc_pcn_mutate and asmc_pcn_mutate_flow, once per call and before anything is launched.  `fn`: the exported
// function's name, the prefix of the error text.
static int pcn_check_call(const char* fn, const asmc_ctx* ctx, int64_t n, const void* x, const double* ll, const double* lp, const double* lq,
                          const asmc_pcn_params* prm, int n_steps, const double* rho_inout_host, const int64_t* n_accept_host,
                          const PcnNeeds& need) {
#define PCN_CALL_REQUIRE(cond, msg)                \
    do {                                           \
        if (!(cond)) {                             \
            asmc_set_error("%s: %s", fn, msg);     \
            return ASMC_ERR_ARG;                   \
        }                                          \
    } while (0)
    PCN_CALL_REQUIRE(ctx && x && ll && lp && lq && prm && rho_inout_host && n_accept_host && (!need.work || need.work_dev), "null pointer");
    PCN_CALL_REQUIRE(n > 0 && n <= ctx->n_max, "n out of range for this ctx");
    PCN_CALL_REQUIRE(n_steps >= 1 && n_steps <= ASMC_MAX_PCN_STEPS, "n_steps out of range (<= 2048 per call)");
    PCN_CALL_REQUIRE(prm->d > 0 && prm->d <= ASMC_MAX_DIMS && (!need.flow || prm->d == need.flow->dims), "bad d");
    PCN_CALL_REQUIRE(prm->x_dtype == ASMC_F64 || prm->x_dtype == ASMC_F32, "bad x_dtype");
    PCN_CALL_REQUIRE(prm->mu_dev && prm->L_dev && prm->Linv_dev, "null reference-Gaussian pointer");
    PCN_CALL_REQUIRE(*rho_inout_host > 0.0 && *rho_inout_host <= 1.0, "rho must be in (0, 1]");
    PCN_CALL_REQUIRE(!need.work || need.work_bytes >= asmc_pcn_flow_work_bytes(n, prm->d, prm->x_dtype), "work buffer too small");
    PCN_CALL_REQUIRE(!(prm->nu > 0.0) || prm->nu >= 1.0, "nu must be >= 1 (or <= 0 for the Gaussian reference)");
    int rc = check_mixture(prm->log_likelihood);
    if (!rc) rc = check_mixture(prm->log_prior);
    if (!rc && need.n_mix == 3) rc = check_mixture(prm->log_q);
    if (rc) return rc;
    PCN_CALL_REQUIRE(!need.noise || prm->noise == ASMC_NOISE_F64 || prm->noise == ASMC_NOISE_F32, "bad noise mode");
#undef PCN_CALL_REQUIRE
    return ASMC_OK;
}

// A device-side loop of Markov steps.  Step t (Philox step index step0 + t): the step's scale variates (tpCN) -> `launch(t, step,
// &grid)`, the step's kernel(s), which yields the grid -> `close(t, grid)`: count, history, adaptation -> `record(t)`.
// pcn_close(loop, counts) - `counts`: where the step's blocks left their accept counts - is the close of every loop but the
// fused flow step's, whose last block adapts by itself; asmc_pcn_mutate alone passes a recorder.
struct PcnLoop {
    asmc_ctx* ctx;
    int64_t n;
    const asmc_pcn_params* prm;
    int n_steps;
    uint32_t step0;
    hipStream_t st;
};

static int pcn_no_record(int) { return ASMC_OK; }

template <typename Launch, typename Close, typename Record = int (*)(int)>
static int pcn_steps(const PcnLoop& lp, PcnDev& pd, Launch&& launch, Close&& close, Record&& record = pcn_no_record) {
    for (int t = 0; t < lp.n_steps; t++) {
        const uint32_t step = lp.step0 + (uint32_t)t;
        int rc = pcn_prepare_gamma(lp.ctx, lp.n, pd, step, lp.st);
        if (rc) return rc;
        int grid = 0;
        rc = launch(t, step, &grid);
        if (rc) return rc;
        rc = close(t, grid);
        if (rc) return rc;
        rc = record(t);
        if (rc) return rc;
    }
    return ASMC_OK;
}

static auto pcn_close(const PcnLoop& lp, const long long* counts) {
    return [&lp, counts](int t, int grid) {
        return pcn_close_step(lp.ctx, lp.st, grid, counts, lp.n, t, lp.ctx->d_counts, lp.ctx->d_rho, lp.ctx->d_rho + 8, lp.prm->target_accept,
                              lp.prm->adapt, t == lp.n_steps - 1);
    };
}

// where the step kernels of a call leave their per-block accept counts
static long long* pcn_block_counts(asmc_ctx* ctx) { return ctx->d_counts + ASMC_MAX_PCN_STEPS; }

// waits for a call's read-back - for `ev` when given, else for the stream - and hands it out (flags: pcn_readback_handout)
static int pcn_collect(asmc_ctx* ctx, int n_steps, bool flow, bool lq_checked, double* rho_out_host, int64_t* n_accept_host,
                       double* rho_hist_host, hipStream_t st, hipEvent_t ev = nullptr) {
    if (ev)
        ASMC_HIP(hipEventSynchronize(ev));
    else
        ASMC_HIP(hipStreamSynchronize(st));
    pcn_readback_handout(ctx, n_steps, flow, lq_checked, rho_out_host, n_accept_host, rho_hist_host);
    return ASMC_OK;
}

// The tail of a mutation call: read-back (counts | step sizes | rho, and *d_bad of a flow mutation: `flow`), the NaN count of the
// carried log q (lq != NULL: `lq_checked`), then the wait and the hand-out - or, `defer`: the results wait in pinned memory for
// asmc_pcn_mutate_flow_result.
static int pcn_finish_call(asmc_ctx* ctx, int64_t n, const double* lq, int n_steps, const void* d_bad, bool defer, double* rho_out_host,
                           int64_t* n_accept_host, double* rho_hist_host, hipStream_t st) {
    int rc = pcn_readback_enqueue(ctx, n_steps, d_bad, st);
    if (rc) return rc;
    if (lq) {
        rc = pcn_enqueue_lq_check(ctx, n, lq, st);
        if (rc) return rc;
    }
    if (defer) {
        if (!ctx->ev_mutate) ASMC_HIP(hipEventCreateWithFlags(&ctx->ev_mutate, hipEventDisableTiming));
        ASMC_HIP(hipEventRecord(ctx->ev_mutate, st));  // _result waits for THIS point, not for what the caller enqueues behind it
        ctx->mutate_pending_steps = n_steps;
        return ASMC_OK;
    }
    return pcn_collect(ctx, n_steps, d_bad != nullptr, lq != nullptr, rho_out_host, n_accept_host, rho_hist_host, st);
}

// ==== asmc_pcn_mutate =======================================================================================================
// d_noise > 0: a d_noise-dimensional problem zero-padded to prm->d (x: the padded copy)
static int pcn_mutate_impl(asmc_ctx* ctx, int64_t n, void* x, double* ll, double* lp, double* lq, const asmc_pcn_params* prm,
                           int n_steps, uint32_t step0, double* rho_inout_host, int64_t* n_accept_host, double* rho_hist_host,
                           asmc_stream stream, int d_noise) {
    const asmc_chain_target& ch = ctx->chain;
    const bool padded = d_noise != 0;  // (then prm->d is the padded width and x the padded copy)
    const size_t row_bytes = (size_t)prm->d * (prm->x_dtype == ASMC_F64 ? 8 : 4);
    if (ctx->chain_on) {  // asmc_chain_set: every recorded slot of this call inside the chain
        ASMC_REQUIRE(ch.n == n && ch.d == (padded ? d_noise : prm->d) && ch.x_dtype == prm->x_dtype, "chain target: n, d or dtype differ from the call's");
        ASMC_REQUIRE(ch.slot0 >= 0 && ch.slot0 + n_steps / ch.stride <= ch.n_slots, "chain target: the call's steps do not fit the chain");
        ASMC_REQUIRE(!padded || ctx->chain_rows_bytes >= (size_t)n * row_bytes, "chain target: no scratch for the padded rows");
    }
    hipStream_t st = as_stream(stream);
    PcnDev pd = pcn_dev_from_params(ctx, prm, d_noise);
    pd.ll = to_dev(prm->log_likelihood);
    pd.lp = to_dev(prm->log_prior);
    pd.lq = to_dev(prm->log_q);
    pd.noise = prm->noise;
    pd.mode = PCN_X_STEP;
    double* d_rho = ctx->d_rho;  // [0]: current rho, [8 ..]: history
    long long* d_block = pcn_block_counts(ctx);
    const PcnLoop loop = {ctx, n, prm, n_steps, step0, st};
    const bool dbg = getenv("ASMC_DEBUG_TIMING") != nullptr;
    auto now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_a = now();
    ASMC_HIP(hipStreamSynchronize(st));
    const double t_b = now();
    ctx->h_pinned[HP_FRONT] = *rho_inout_host;
    ASMC_HIP(hipMemcpyAsync(d_rho, ctx->h_pinned, sizeof(double), hipMemcpyHostToDevice, st));
    // Slot of step t of this call (asmc_chain_set).  Not whitened: the rows are x itself (un-padded on their way when the call
    // runs on a zero-padded copy).  Whitened: the call's own un-whitening launch `unwhiten(rec)` with the slot's rows (the padded
    // scratch, un-padded behind it) and density rows as its outputs rec[0 .. 3]; a launch that un-whitens x where it lies
    // (`in_place`: the matrix-core and the row-major register kernels) gets a copy of the state there first.  The state itself is
    // only read.  These are the launches that end a call of t + 1 steps: the same bits.
    auto record_state = [&](int t, bool whitened, bool in_place, auto&& unwhiten) -> int {
        const int64_t slot = ch.slot0 + t / ch.stride;
        char* slot_x = static_cast<char*>(ch.x_dev) + (size_t)slot * (size_t)n * (size_t)ch.pitch * (row_bytes / prm->d);
        if (!whitened) {
            if (!padded) return asmc_chain_rows_launch(ctx, &ch, slot, x, ll, lp, st);
            const int r = launch_unpad_rows(ctx, n, d_noise, prm->d, prm->x_dtype, x, slot_x, st);
            return r ? r : asmc_chain_scalars_launch(ctx, &ch, slot, ll, lp, st);
        }
        void* dst = padded ? ctx->d_chain_rows : slot_x;
        if (in_place) ASMC_HIP(hipMemcpyAsync(dst, x, (size_t)n * row_bytes, hipMemcpyDeviceToDevice, st));
        void* rec[4] = {dst, ch.ll_dev + (size_t)slot * (size_t)n, ch.lp_dev + (size_t)slot * (size_t)n, ctx->d_chain_lq};
        const int r = unwhiten(rec);
        if (r || !padded) return r;
        return launch_unpad_rows(ctx, n, d_noise, prm->d, prm->x_dtype, dst, slot_x, st);
    };
    // A path of the call: `launch(op, step, &grid, rec)` is its kernel for the three operations; `rec` != NULL: the launch works on
    // rec[0] (rows) and rec[1 .. 3] (ll, lp, lq) instead of the population's arrays - the chain recorder's use of the un-whitening
    // epilogue (record_state).  `whitened`: the steps run between a whitening and an un-whitening launch; `in_place`: see record_state.
    enum { OP_WHITEN, OP_STEP, OP_UNWHITEN };
    auto run = [&](bool whitened, bool in_place, auto&& launch) -> int {
        int grid = 0;
        int rc = whitened ? launch(OP_WHITEN, 0, &grid, nullptr) : ASMC_OK;
        if (rc) return rc;
        rc = pcn_steps(
            loop, pd,
            [&](int, uint32_t step, int* g) { return launch(OP_STEP, step, g, nullptr); }, pcn_close(loop, d_block),
            [&](int t) -> int {
                if (!(ctx->chain_on && t % ch.stride == ch.stride - 1)) return ASMC_OK;
                return record_state(t, whitened, in_place, [&](void* const* rec) -> int {
                    int g2 = 0;
                    return launch(OP_UNWHITEN, 0, &g2, rec);
                });
            });
        if (rc) return rc;
        return whitened ? launch(OP_UNWHITEN, 0, &grid, nullptr) : ASMC_OK;
    };
    const bool mm = asmc_pcn_mm_supported(pd.d, x) && !pcn_env_generic();
    int rc;
    if (mm) {
        // d = 64 / 128: triangular mat-vecs on the fp64 matrix cores, always on the whitened state
        rc = asmc_pcn_mm_pack(ctx, pd, st);
        if (rc) return rc;
        rc = run(true, true, [&](int op, uint32_t stp, int* grid, void* const* rec) {
            const int mode = op == OP_WHITEN ? MM_WHITEN : op == OP_UNWHITEN ? MM_UNWHITEN : pd.nu > 0.0 ? MM_STEP_T : MM_STEP;
            return asmc_pcn_mm_launch(ctx, n, prm->x_dtype, rec ? rec[0] : x, rec ? (double*)rec[1] : ll, rec ? (double*)rec[2] : lp,
                                      rec ? (double*)rec[3] : lq, pd, mode, d_rho, stp, d_block, grid, st);
        });
    } else {
        const bool reg_ok = pcn_reg_supported(pd.d, prm->x_dtype == ASMC_F64 ? 8 : 4, x);
        // whitened-state stepping: plain (single-component) targets, enough steps to amortise the two conversions
        const bool single = pd.ll.C == 1 && pd.lp.C == 1 && pd.lq.C == 1;
        bool y_state = reg_ok && n_steps >= 4 && !pcn_env_xstate();  // several components: only coordinate-major (below)
        // whitened state in a coordinate-major scratch buffer (grown on demand, kept for the life of the ctx)
        const bool soa = y_state && pcn_ensure_ysoa(ctx, n, pd.d, prm->x_dtype, pd, st);
        if (!single && !soa) y_state = false;  // the row-major whitened-state kernel folds single Gaussians only
        const bool tp = pd.nu > 0.0 && reg_ok;  // the generic kernel branches on the variates' pointer at run time
        if (reg_ok) {
            rc = pack_pcn_tables(ctx, pd, st);
            if (rc) return rc;
        }
        rc = run(y_state, y_state && !soa, [&](int op, uint32_t stp, int* grid, void* const* rec) {
            int mode = op == OP_WHITEN ? PCN_WHITEN : op == OP_UNWHITEN ? PCN_UNWHITEN
                       : y_state ? (tp ? PCN_Y_STEP_T : PCN_Y_STEP) : (tp ? PCN_X_STEP_T : PCN_X_STEP);
            if (soa) mode = mode == PCN_WHITEN ? PCN_WHITEN_S : mode == PCN_UNWHITEN ? PCN_UNWHITEN_S
                            : mode == PCN_Y_STEP ? (single ? PCN_Y_STEP_S : PCN_Y_STEP_SG)
                            : mode == PCN_Y_STEP_T ? (single ? PCN_Y_STEP_TS : PCN_Y_STEP_TSG) : mode;
            pd.mode = mode;
            const int nz = pd.noise;
            if (op != OP_STEP) pd.noise = ASMC_NOISE_F64;  // (the conversions draw nothing: they are instantiated under this key only)
            const int r = pcn_step_launch(ctx, n, prm->x_dtype, rec ? rec[0] : x, rec ? (double*)rec[1] : ll, rec ? (double*)rec[2] : lp,
                                          rec ? (double*)rec[3] : lq, pd, d_rho, stp, d_block, grid, st);
            pd.noise = nz;
            return r;
        });
    }
    if (rc) return rc;
    const double t_c = now();
    rc = pcn_finish_call(ctx, n, lq, n_steps, nullptr, false, rho_inout_host, n_accept_host, rho_hist_host, st);
    if (rc) return rc;
    if (dbg && !mm)  // (the register and generic paths' line; the matrix-core path has never printed one)
        fprintf(stderr, "[asmc_pcn_mutate] sync0 %.3f ms, enqueue %.3f ms, drain %.3f ms (n_steps=%d)\n", t_b - t_a, t_c - t_b, now() - t_c, n_steps);
    return ASMC_OK;
}

static int pcn_mutate_padded(asmc_ctx* ctx, int64_t n, void* x, double* ll, double* lp, double* lq, const asmc_pcn_params* prm,
                             int D, int n_steps, uint32_t step0, double* rho_inout_host, int64_t* n_accept_host,
                             double* rho_hist_host, asmc_stream stream) {
    hipStream_t st = as_stream(stream);
    asmc_pcn_params p2;
    void* xp = nullptr;
    int rc = pcn_pad_params(ctx, n, x, prm, D, 3, st, &p2, &xp);
    if (rc) return rc;
    rc = pcn_mutate_impl(ctx, n, xp, ll, lp, lq, &p2, n_steps, step0, rho_inout_host, n_accept_host, rho_hist_host, stream, prm->d);
    if (rc) return rc;
    return launch_unpad_rows(ctx, n, prm->d, D, prm->x_dtype, xp, x, st);
}

extern "C" {

int asmc_pcn_mutate(asmc_ctx* ctx, int64_t n, void* x, double* ll, double* lp, double* lq,
                    const asmc_pcn_params* prm, int n_steps, uint32_t step0, double* rho_inout_host,
                    int64_t* n_accept_host, double* rho_hist_host, asmc_stream stream) {
    int rc = pcn_check_call(__func__, ctx, n, x, ll, lp, lq, prm, n_steps, rho_inout_host, n_accept_host, {3, true, nullptr, false, nullptr, 0});
    if (!rc) rc = pcn_generic_check(prm->d, prm->x_dtype);  // (before the Gamma draw of a tpCN step)
    if (rc) return rc;
    const int D = pcn_pad_dim(prm->d);
    const bool fast_as_is = prm->d == D;
    if (!fast_as_is && D > 0 && D <= ctx->d_max_pad && !pcn_env_generic() && !pcn_env_nopad())
        return pcn_mutate_padded(ctx, n, x, ll, lp, lq, prm, D, n_steps, step0, rho_inout_host, n_accept_host, rho_hist_host, stream);
    return pcn_mutate_impl(ctx, n, x, ll, lp, lq, prm, n_steps, step0, rho_inout_host, n_accept_host, rho_hist_host, stream, 0);
}

}  // extern "C"

// ==== the split path: asmc_pcn_propose / _accept / _split_*, the whitened-state session asmc_pcn_ysplit_* ===================
// proposal half of the split path for the step `step` (gamma variates drawn first when pd.nu > 0): register-resident
// kernel for d in {4, 8, 16, 32}, the same kernel on identity-padded tables for 16 < d < 32, generic LDS kernel otherwise
static int pcn_propose_launch(asmc_ctx* ctx, int64_t n, int d, int x_dtype, const void* x, void* x_prop, double* qf_old,
                              double* qf_new, PcnDev pd, const double* rho_ptr, uint32_t step, hipStream_t st) {
    int grid = 0;
    int rc = pcn_prepare_gamma(ctx, n, pd, step, st);
    if (rc) return rc;
    const bool pad = d > 16 && d < 32 && !pcn_env_generic();
    if (pad || (pcn_reg_supported(d, x_dtype == ASMC_F64 ? 8 : 4, x) && ((uintptr_t)x_prop % 16) == 0)) {
        // d in {4, 8, 16, 32}: the register-resident kernel's proposal half (same arithmetic as the fused step);
        // 16 < d < 32: the same kernel compiled for 32 dimensions with identity-padded tables
        pd.dpad = pad ? 32 : 0;
        pd.mode = pad ? (pd.nu > 0.0 ? PCN_X_PROPOSE_PAD_T : PCN_X_PROPOSE_PAD) : (pd.nu > 0.0 ? PCN_X_PROPOSE_T : PCN_X_PROPOSE);
        pd.noise = ASMC_NOISE_F64;
        pd.ys = x_prop;
        rc = pack_pcn_tables(ctx, pd, st);
        if (rc) return rc;
        return pcn_step_launch(ctx, n, x_dtype, const_cast<void*>(x), qf_old, qf_new, nullptr, pd, rho_ptr, step, nullptr, &grid, st);
    }
    if (asmc_pcn_mm_supported(d, x) && ((uintptr_t)x_prop % 16) == 0 && ctx->d_mmtab && !pcn_env_generic()) {
        // d = 64 / 128: both mat-vecs of the proposal on the fp64 matrix cores (the generic LDS kernel took 10 / 76 ms per
        // step at 1M particles - the path every user with Python densities and d > 32 was on)
        pd.noise = ASMC_NOISE_F64;
        rc = asmc_pcn_mm_pack(ctx, pd, st);
        if (rc) return rc;
        return asmc_pcn_mm_launch(ctx, n, x_dtype, const_cast<void*>(x), qf_old, qf_new, reinterpret_cast<double*>(x_prop), pd,
                                  pd.nu > 0.0 ? MM_XPROPOSE_T : MM_XPROPOSE, rho_ptr, step, nullptr, &grid, st);
    }
    const int D = pcn_pad_dim(d);
    if (D != d && D > 0 && D <= ctx->d_max_pad && !(D == 32 && d > 16) && !pcn_env_generic() && !pcn_env_nopad()) {
        // any other d <= 128 (17 .. 31 have the in-kernel padding above): zero-padded copies of the rows and of the reference's
        // tables, the D-dimensional proposal kernel with the noise masked beyond d, x' copied back without the padding
        PcnDev src = pd;
        src.ll.C = src.lp.C = src.lq.C = 0;
        PcnPadded pad;
        rc = pcn_pad_problem(ctx, n, d, D, x_dtype, x, src, 0, st, &pad);
        if (rc) return rc;
        PcnDev p2 = pd;
        p2.d = D;
        p2.d_noise = d;
        p2.mu = pad.mu;
        p2.L = pad.L;
        p2.Linv = pad.Linv;
        rc = pcn_propose_launch(ctx, n, D, x_dtype, pad.xp, pad.xq, qf_old, qf_new, p2, rho_ptr, step, st);
        if (rc) return rc;
        return launch_unpad_rows(ctx, n, d, D, x_dtype, pad.xq, x_prop, st);
    }
    return pcn_generic_propose_launch(ctx, n, x_dtype, x, x_prop, qf_old, qf_new, pd, rho_ptr, step, &grid, st);
}

// ---- whitened-state session of the split path (asmc.h) -----------------------------------------------------------------
static int ysplit_pd(asmc_ctx* ctx, int64_t n, const asmc_pcn_params* prm, PcnDev& pd) {
    ASMC_REQUIRE(ctx && prm, "null pointer");
    ASMC_REQUIRE(n > 0 && n <= ctx->n_max, "n out of range for this ctx");
    ASMC_REQUIRE(prm->x_dtype == ASMC_F64 || prm->x_dtype == ASMC_F32, "bad x_dtype");
    ASMC_REQUIRE(prm->mu_dev && prm->L_dev && prm->Linv_dev, "null reference pointer");
    ASMC_REQUIRE(!(prm->nu > 0.0) || prm->nu >= 1.0, "nu must be >= 1 (or <= 0 for the Gaussian reference)");
    pd = pcn_dev_from_params(ctx, prm, 0);  // (no built-in densities: the caller evaluates its own between propose and accept)
    ASMC_REQUIRE(prm->noise == ASMC_NOISE_F64 || prm->noise == ASMC_NOISE_F32, "bad noise mode");
    pd.noise = prm->noise;  // same in every call of a session: accept regenerates what propose drew
    return ASMC_OK;
}

// the open session's state and tables for a proposal: pd.ys / pd.n_pad, the tables packed again when someone else packed
// parameter tables on this context since asmc_pcn_ysplit_begin (cheap insurance; a context carries ONE mutation at a time - step
// size, counts and scale variates are per context - see include/asmc.h), the step's scale variates
static int ysplit_propose_prepare(asmc_ctx* ctx, int64_t n, PcnDev& pd, uint32_t step, hipStream_t st) {
    pd.ys = ctx->d_ysoa;
    pd.n_pad = ((n + 63) / 64) * 64;
    if (ctx->ptab_tag == 0 || ctx->ptab_tag != ctx->ysplit_seq) {
        const int rc = pack_pcn_tables(ctx, pd, st);
        if (rc) return rc;
        ctx->ptab_tag = ctx->ysplit_seq;
    }
    return pcn_prepare_gamma(ctx, n, pd, step, st);
}

extern "C" {

int asmc_pcn_propose(asmc_ctx* ctx, int64_t n, int d, int x_dtype, const void* x, void* x_prop, double* qf_old,
                     double* qf_new, const double* mu, const double* L, const double* Linv, double rho, double nu,
                     uint64_t seed, uint64_t gid0, uint32_t step, asmc_stream stream) {
    ASMC_REQUIRE(ctx && x && x_prop && qf_old && qf_new && mu && L && Linv, "null pointer");
    ASMC_REQUIRE(!(nu > 0.0) || nu >= 1.0, "nu must be >= 1 (or <= 0 for the Gaussian reference)");
    ASMC_REQUIRE(n > 0 && n <= ctx->n_max && d > 0 && d <= ASMC_MAX_DIMS, "bad sizes");
    ASMC_REQUIRE(x_dtype == ASMC_F64 || x_dtype == ASMC_F32, "bad x_dtype");
    ASMC_REQUIRE(rho >= 0.0 && rho <= 1.0, "rho must be in (0, 1], or 0 for the device-resident step size");
    const int fits = pcn_generic_check(d, x_dtype);
    if (fits) return fits;
    hipStream_t st = as_stream(stream);
    PcnDev pd;
    memset(&pd, 0, sizeof(pd));
    pd.bmtab = ctx->d_bmtab;
    pd.d = d;
    pd.mu = mu;
    pd.L = L;
    pd.Linv = Linv;
    pd.seed = seed;
    pd.gid0 = gid0;
    pd.nu = nu;
    if (rho > 0.0) {  // by kernel argument: no pinned staging, no synchronisation
        const int rc = pcn_set_scalar_launch(ctx, ctx->d_rho, rho, st);
        if (rc) return rc;
    }
    return pcn_propose_launch(ctx, n, d, x_dtype, x, x_prop, qf_old, qf_new, pd, ctx->d_rho, step, st);
}

// Split path without a host round trip per step (asmc.h): the step size lives in the ctx, asmc_pcn_accept leaves its
// count on the device, asmc_pcn_split_adapt closes the step like the fused loops do (exchange hook included).
int asmc_pcn_split_begin(asmc_ctx* ctx, double rho0, asmc_stream stream) {
    ASMC_REQUIRE(ctx != nullptr, "null ctx");
    ASMC_REQUIRE(rho0 > 0.0 && rho0 <= 1.0, "rho must be in (0, 1]");
    return pcn_set_scalar_launch(ctx, ctx->d_rho, rho0, as_stream(stream));
}

int asmc_pcn_split_adapt(asmc_ctx* ctx, int64_t n_global, double target_accept, int t, int adapt, asmc_stream stream) {
    ASMC_REQUIRE(ctx != nullptr, "null ctx");
    ASMC_REQUIRE(n_global > 0 && t >= 0 && t < ASMC_MAX_PCN_STEPS, "bad n_global / step index");
    hipStream_t st = as_stream(stream);
    // the accept kernel's count cell (d_keys[0]) plays the part of a one-block partial
    return pcn_close_step(ctx, st, 1, reinterpret_cast<const long long*>(ctx->d_keys), n_global, t, ctx->d_counts, ctx->d_rho,
                          ctx->d_rho + 8, target_accept, adapt);
}

int asmc_pcn_split_end(asmc_ctx* ctx, int n_steps, int64_t* n_accept_host, double* rho_hist_host, double* rho_host,
                       asmc_stream stream) {
    ASMC_REQUIRE(ctx && n_accept_host && rho_host, "null pointer");
    ASMC_REQUIRE(n_steps >= 1 && n_steps <= ASMC_MAX_PCN_STEPS, "n_steps out of range");
    hipStream_t st = as_stream(stream);
    ASMC_HIP(hipStreamSynchronize(st));  // pinned staging may still be in flight
    return pcn_finish_call(ctx, 0, nullptr, n_steps, nullptr, false, rho_host, n_accept_host, rho_hist_host, st);
}

int asmc_pcn_ysplit_begin(asmc_ctx* ctx, int64_t n, const void* x, const asmc_pcn_params* prm, double rho0,
                          asmc_stream stream) {
    PcnDev pd;
    int rc = ysplit_pd(ctx, n, prm, pd);
    if (rc) return rc;
    ASMC_REQUIRE(x != nullptr, "null pointer");
    ASMC_REQUIRE(rho0 > 0.0 && rho0 <= 1.0, "rho must be in (0, 1]");
    hipStream_t st = as_stream(stream);
    if (!pcn_reg_supported(pd.d, prm->x_dtype == ASMC_F64 ? 8 : 4, x) || !pcn_ensure_ysoa(ctx, n, pd.d, prm->x_dtype, pd, st)) {
        asmc_set_error("whitened-state split session: d=%d is not a register-kernel dimension or no scratch", pd.d);
        return ASMC_ERR_UNSUPPORTED;
    }
    rc = pcn_set_scalar_launch(ctx, ctx->d_rho, rho0, st);
    if (rc) return rc;
    rc = pack_pcn_tables(ctx, pd, st);
    if (rc) return rc;
    ctx->ptab_tag = ++ctx->ysplit_seq;
    pd.mode = PCN_WHITEN_S;
    pd.noise = ASMC_NOISE_F64;  // (the whitening kernels draw nothing: they are instantiated under this key only)
    int grid = 0;
    return pcn_step_launch(ctx, n, prm->x_dtype, const_cast<void*>(x), nullptr, nullptr, nullptr, pd, ctx->d_rho, 0, pcn_block_counts(ctx),
                           &grid, st);
}

int asmc_pcn_ysplit_propose(asmc_ctx* ctx, int64_t n, const asmc_pcn_params* prm, uint32_t step, void* x_prop,
                            asmc_stream stream) {
    PcnDev pd;
    int rc = ysplit_pd(ctx, n, prm, pd);
    if (rc) return rc;
    ASMC_REQUIRE(x_prop != nullptr && ((uintptr_t)x_prop % 16) == 0, "x_prop must be a 16-byte aligned device buffer");
    ASMC_REQUIRE(ctx->d_ysoa != nullptr, "no session (asmc_pcn_ysplit_begin)");
    hipStream_t st = as_stream(stream);
    rc = ysplit_propose_prepare(ctx, n, pd, step, st);
    if (rc) return rc;
    int grid = 0;
    return pcn_reg_flow_launch(ctx, n, prm->x_dtype, PCN_FLOW_PROPOSE_SX, nullptr, x_prop, nullptr, nullptr, nullptr, nullptr, nullptr,
                               nullptr, pd, ctx->d_rho, step, pcn_block_counts(ctx), &grid, st);
}

int asmc_pcn_ysplit_propose_tr(asmc_ctx* ctx, int64_t n, const asmc_pcn_params* prm, uint32_t step, const asmc_transform* t,
                               const double* premap_dev, const asmc_mixture* qmix, int minus_logj, void* x_prop,
                               double* logj_out, double* lq_out, asmc_stream stream) {
    PcnDev pd;
    int rc = ysplit_pd(ctx, n, prm, pd);
    if (rc) return rc;
    ASMC_REQUIRE(t && x_prop && logj_out && ((uintptr_t)x_prop % 16) == 0, "null / misaligned pointer");
    ASMC_REQUIRE(ctx->d_ysoa != nullptr, "no session (asmc_pcn_ysplit_begin)");
    ASMC_REQUIRE(t->d == pd.d && t->kind_dev && t->lower_dev && t->upper_dev, "transform tables missing or of another dimension");
    ASMC_REQUIRE((t->mean_dev == nullptr) == (t->std_dev == nullptr), "affine stage needs both mean and std");
    ASMC_REQUIRE((premap_dev == nullptr) == (qmix == nullptr) && (premap_dev == nullptr) == (lq_out == nullptr),
                 "premap, mixture and lq_out come together");
    ASMC_REQUIRE(!qmix || qmix->n_components == 1, "the proposal density must be a single Gaussian");
    const int logit = (t->hints & 7) == (ASMC_TR_NO_PERIODIC | ASMC_TR_NO_PROBIT);
    const int probit = (t->hints & 7) == (ASMC_TR_NO_PERIODIC | ASMC_TR_NO_LOGIT);
    if (!logit && !probit) {
        asmc_set_error("asmc_pcn_ysplit_propose_tr: the transform must be non-periodic with ONE bounded stage (hints %d)", t->hints);
        return ASMC_ERR_UNSUPPORTED;
    }
    hipStream_t st = as_stream(stream);
    rc = ysplit_propose_prepare(ctx, n, pd, step, st);
    if (rc) return rc;
    double* d_tab = ctx->d_small + DS_TRTAB;  // DS_TRTAB_LEN doubles
    rc = pcn_trtab_pack_launch(ctx, pd.d, t, premap_dev, qmix, minus_logj, d_tab, st);
    if (rc) return rc;
    int grid = 0;
    return pcn_reg_flow_launch(ctx, n, prm->x_dtype, logit ? PCN_FLOW_PROPOSE_SXT_LOGIT : PCN_FLOW_PROPOSE_SXT_PROBIT, nullptr, x_prop,
                               nullptr, nullptr, nullptr, logj_out, lq_out, d_tab, pd, ctx->d_rho, step, pcn_block_counts(ctx), &grid, st);
}

int asmc_pcn_ysplit_accept(asmc_ctx* ctx, int64_t n, const asmc_pcn_params* prm, uint32_t step, double* ll, double* lp,
                           double* lq, const double* ll_new, const double* lp_new, const double* lq_new, double* lj,
                           const double* lj_new, int64_t n_global, int t, asmc_stream stream) {
    PcnDev pd;
    int rc = ysplit_pd(ctx, n, prm, pd);
    if (rc) return rc;
    ASMC_REQUIRE(ll && lp && lq && ll_new && lp_new && lq_new, "null pointer");
    ASMC_REQUIRE((lj == nullptr) == (lj_new == nullptr), "log-Jacobian arrays: both or neither");
    ASMC_REQUIRE(ctx->d_ysoa != nullptr, "no session (asmc_pcn_ysplit_begin)");
    ASMC_REQUIRE(n_global > 0 && t >= 0 && t < ASMC_MAX_PCN_STEPS, "bad n_global / step index");
    hipStream_t st = as_stream(stream);
    pd.ys = ctx->d_ysoa;
    pd.n_pad = ((n + 63) / 64) * 64;
    rc = pcn_prepare_gamma(ctx, n, pd, step, st);  // the variates asmc_pcn_ysplit_propose drew for this step (still there; else redrawn: counter based)
    if (rc) return rc;
    int grid = 0;
    long long* d_block = pcn_block_counts(ctx);
    // with a carried log-Jacobian the two arrays travel through the kernel's y / x_prop parameters (PCN_FLOW_ACCEPT_SJ)
    rc = pcn_reg_flow_launch(ctx, n, prm->x_dtype, lj ? PCN_FLOW_ACCEPT_SJ : PCN_FLOW_ACCEPT_S, lj, const_cast<double*>(lj_new), ll, lp, lq,
                             const_cast<double*>(ll_new), const_cast<double*>(lp_new), lq_new, pd, ctx->d_rho, step, d_block, &grid, st);
    if (rc) return rc;
    return pcn_close_step(ctx, st, grid, d_block, n_global, t, ctx->d_counts, ctx->d_rho, ctx->d_rho + 8, prm->target_accept,
                          prm->adapt);
}

}  // extern "C"

// y -> x_out [n, d] of the open session (the state is only read): asmc_pcn_ysplit_end's launch, and the chain recorder's
int asmc_pcn_ysplit_unwhiten(asmc_ctx* ctx, int64_t n, void* x, const asmc_pcn_params* prm, bool repack, hipStream_t st) {
    PcnDev pd;
    int rc = ysplit_pd(ctx, n, prm, pd);
    if (rc) return rc;
    ASMC_REQUIRE(x != nullptr && ctx->d_ysoa != nullptr, "null pointer / no session");
    ASMC_REQUIRE(repack || pcn_reg_supported(pd.d, prm->x_dtype == ASMC_F64 ? 8 : 4, x), "x_out: a 16-byte aligned buffer of a session's d");
    pd.ys = ctx->d_ysoa;
    pd.n_pad = ((n + 63) / 64) * 64;
    pd.mode = PCN_UNWHITEN_XS;
    pd.noise = ASMC_NOISE_F64;
    if (repack || ctx->ptab_tag == 0 || ctx->ptab_tag != ctx->ysplit_seq) {
        rc = pack_pcn_tables(ctx, pd, st);
        if (rc) return rc;
        if (!repack) ctx->ptab_tag = ctx->ysplit_seq;  // (as asmc_pcn_ysplit_propose: the session's tables are back)
    }
    int grid = 0;
    return pcn_step_launch(ctx, n, prm->x_dtype, x, nullptr, nullptr, nullptr, pd, ctx->d_rho, 0, pcn_block_counts(ctx), &grid, st);
}

extern "C" {

int asmc_pcn_ysplit_end(asmc_ctx* ctx, int64_t n, void* x, const asmc_pcn_params* prm, asmc_stream stream) {
    return asmc_pcn_ysplit_unwhiten(ctx, n, x, prm, true, as_stream(stream));
}

int asmc_pcn_accept(asmc_ctx* ctx, int64_t n, int d, int x_dtype, void* x, const void* x_prop, double* ll, double* lp,
                    double* lq, const double* ll_new, const double* lp_new, const double* lq_new,
                    double* lj_old, const double* lj_new, const double* qf_old, const double* qf_new,
                    double beta, uint64_t seed, uint64_t gid0, uint32_t step, int64_t* n_accept_host,
                    asmc_stream stream) {
    ASMC_REQUIRE(ctx && x && x_prop && ll && lp && lq && ll_new && lp_new && lq_new && qf_old && qf_new, "null pointer");
    ASMC_REQUIRE(n > 0 && n <= ctx->n_max && d > 0, "bad sizes");
    ASMC_REQUIRE(x_dtype == ASMC_F64 || x_dtype == ASMC_F32, "bad x_dtype");
    hipStream_t st = as_stream(stream);
    int rc = pcn_accept_flags_launch(ctx, n, ll, lp, lq, ll_new, lp_new, lq_new, lj_old, lj_new, qf_old, qf_new, beta, seed, gid0, step, st);
    if (rc) return rc;
    rc = launch_copy_flagged(ctx, n, d, x_dtype, x, x_prop, ctx->d_flags, st);
    if (rc) return rc;
    if (n_accept_host) {
        unsigned long long* h = reinterpret_cast<unsigned long long*>(ctx->h_pinned);
        ASMC_HIP(hipMemcpyAsync(h, ctx->d_keys, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        ASMC_HIP(hipStreamSynchronize(st));
        *n_accept_host = (int64_t)h[0];
    }
    return ASMC_OK;
}

// pCN with a coupling-flow proposal density: per step  propose -> flow log q(x') (fp32 MFMA, asmc_flow.hip) ->
// built-in log prior / log likelihood of x' -> accept -> device-side step-size adaptation; no host round trip
// inside the loop.  Work buffer: x' [n, d] (storage type) | q0 | q1 | ll' | lp' | lq'  (fp64 [n] each).
int64_t asmc_pcn_flow_work_bytes(int64_t n, int d, int x_dtype) {
    const int64_t xb = ((n * d * (x_dtype == ASMC_F64 ? 8 : 4) + 255) / 256) * 256;
    return xb + 5 * (((n * 8 + 255) / 256) * 256);
}

}  // extern "C"

// ==== asmc_pcn_mutate_flow ==================================================================================================
// the non-finite-density counter of a flow mutation's steps (read back with the call's results)
static unsigned long long* pcn_flow_bad_cell(asmc_ctx* ctx) {
    return reinterpret_cast<unsigned long long*>(ctx->d_tilectr + 2 * ASMC_MAX_PCN_STEPS);
}

// d <= 32.  d_noise > 0: a d_noise-dimensional problem zero-padded to prm->d = 32 by asmc_pcn_mutate_flow below (the flow keeps its
// own dims = d_noise); only the one-kernel step takes it
static int pcn_mutate_flow_impl(asmc_ctx* ctx, int64_t n, void* x, double* ll, double* lp, double* lq,
                                const asmc_pcn_params* prm, const asmc_coupling* flow, void* work_dev, int n_steps, uint32_t step0,
                                double* rho_inout_host, int64_t* n_accept_host, double* rho_hist_host, asmc_stream stream, int d_noise) {
    hipStream_t st = as_stream(stream);
    const int d = prm->d;
    const int64_t xb = ((n * d * (prm->x_dtype == ASMC_F64 ? 8 : 4) + 255) / 256) * 256;
    const int64_t vb = ((n * 8 + 255) / 256) * 256;
    char* w = reinterpret_cast<char*>(work_dev);
    void* x_prop = w;
    double* q0 = reinterpret_cast<double*>(w + xb);
    double* q1 = reinterpret_cast<double*>(w + xb + vb);
    double* ll_new = reinterpret_cast<double*>(w + xb + 2 * vb);
    double* lp_new = reinterpret_cast<double*>(w + xb + 3 * vb);
    double* lq_new = reinterpret_cast<double*>(w + xb + 4 * vb);
    PcnDev pd = pcn_dev_from_params(ctx, prm, d_noise);
    double* d_rho = ctx->d_rho;
    long long* d_block = pcn_block_counts(ctx);
    const PcnLoop loop = {ctx, n, prm, n_steps, step0, st};
    int rc;
    // the step size goes to the device as a kernel argument: no pinned staging, so no synchronisation in front of this call's
    // launches - the host enqueues the whole mutation while the reference fit's passes are still running
    // register-resident whitened-state path (d in {4, 8, 16, 32}): x -> y once, then per step
    // propose / flow / accept / adapt, y -> x at the end; four launches per step, no host round trip
    const bool reg_ok = pcn_reg_supported(d, prm->x_dtype == ASMC_F64 ? 8 : 4, x) && !pcn_env_xstate();
    if (reg_ok) {
        pd.ll = to_dev(prm->log_likelihood);
        pd.lp = to_dev(prm->log_prior);
        pd.lq = pd.lp;  // placeholder: the proposal density is the flow
        pd.noise = prm->noise;
        rc = pack_pcn_tables(ctx, pd, st, d_rho, *rho_inout_host);  // (the table pack carries the step size)
        if (rc) return rc;
        int grid = 0;
        const bool soa = pcn_ensure_ysoa(ctx, n, d, prm->x_dtype, pd, st, asmc_pcn_flow_fused_ok(prm, flow));
        auto convert = [&](int mode) -> int {
            PcnDev pc = pd;
            pc.mode = !soa ? mode : mode == PCN_WHITEN ? PCN_WHITEN_S : PCN_UNWHITEN_XS;
            pc.noise = ASMC_NOISE_F64;
            return pcn_step_launch(ctx, n, prm->x_dtype, x, ll, lp, lq, pc, d_rho, 0, d_block, &grid, st);
        };
        rc = convert(PCN_WHITEN);
        if (rc) return rc;
        // one kernel per step (propose -> flow on the MFMA -> targets -> accept) where the shape allows it
        const bool fused = soa && asmc_pcn_flow_fused_ok(prm, flow);
        if (d_noise > 0 && !fused) {
            asmc_set_error("asmc_pcn_mutate_flow: the zero-padded form needs the one-kernel step");
            return ASMC_ERR_UNSUPPORTED;
        }
        if (fused) {
            // counters of the fused steps: [t] tile hand-out, [ASMC_MAX_PCN_STEPS + t] blocks done
            // (sizes in multiples of 16 bytes: a ragged memset is two fill kernels)
            // ... and every tile starts in half 0 of the state allocation (tile parities: the split path's flag bytes,
            // free here, which sit right behind the counters: ONE fill)
            // (beta = 1: the call's `moved` marks, one per PARTICLE, lie behind the parities - asmc_scratch.h - and the fill reaches
            // over them as well)
            const bool at_one = prm->beta == 1.0;
            ASMC_HIP(hipMemsetAsync(ctx->d_tilectr, 0, ASMC_TILECTR_BYTES + scratch_flags_moved_off(n) + (at_one ? scratch_flags_fill(n) : 0), st));
            pd.tile_par = ctx->d_flags;
            int img_words = 0;  // the steps' LDS image, built once per call (0: every step stages for itself)
            rc = asmc_pcn_flow_fused_stage(ctx, pd, flow, &img_words, st);
            if (rc) return rc;
            // beta = 1 EXACTLY: (1 - beta) lq + beta (ll + lp) is 0 * lq + (ll + lp), no accept decision reads the flow density - the
            // steps run without it and one refresh behind the last of them stores log q of the particles that moved
            // (asmc_pcn_fused.hip, FUSED_MODE_NQ / _LQ).  Any other beta, however close: the full step.
            const bool no_density = at_one && asmc_pcn_flow_fused_beta1_ok(flow, img_words);
            const int lag = prm->adapt >= 2 ? prm->adapt : 1;
            rc = pcn_steps(
                loop, pd,
                [&](int t, uint32_t step, int* g) -> int {
                    // single rank: the step's last block adapts the step size itself; sharded: the ranks' counts are exchanged
                    // between the steps and the next step's prologue adapts (PcnAdaptArgs)
                    PcnAdaptArgs ad = {ctx->d_tilectr + ASMC_MAX_PCN_STEPS + t,
                                       reinterpret_cast<unsigned long long*>(ctx->d_tilectr + 2 * ASMC_MAX_PCN_STEPS),
                                       ctx->count_hook ? ctx->count_cell : nullptr,
                                       ctx->count_hook && t > 0 ? ctx->count_cell : nullptr, ctx->d_counts, d_rho, d_rho + 8,
                                       prm->target_accept, ctx->count_hook ? ctx->count_n_global : n, t, prm->adapt, t == n_steps - 1};
                    if (ctx->count_hook && lag > ctx->count_cells) {
                        asmc_set_error("adapt_lag %d needs %d exchange cells, the installed hook has %d (asmc_pcn_set_count_cells)", lag, lag, ctx->count_cells);
                        return ASMC_ERR_ARG;
                    }
                    return asmc_pcn_flow_fused_launch(ctx, n, prm->x_dtype == ASMC_F64 ? ASMC_F64 : ASMC_F32, ll, lp, lq, pd, flow, d_rho, step,
                                                      ctx->d_tilectr + t, d_block, g, ad, img_words, no_density, st);
                },
                [&](int t, int) -> int {
                    // the kernel's last block left this rank's count in the step's cell: exchange it - lagged runs at the end of a block
                    if (!(ctx->count_hook && ((t + 1) % lag == 0 || t == n_steps - 1))) return ASMC_OK;
                    const int hrc = ctx->count_hook(ctx->count_hook_user, reinterpret_cast<asmc_stream>(st));
                    if (hrc != 0) {
                        asmc_set_error("accept-count exchange hook failed (%d)", hrc);
                        return ASMC_ERR_ARG;
                    }
                    // nobody's prologue follows the last step
                    return t == n_steps - 1 ? pcn_adapt_exchanged_launch(ctx, t, prm->target_accept, prm->adapt, lag, st) : ASMC_OK;
                });
            // (in front of the un-whitening and the call's tail: the NaN census of the carried log q and a deferred call's result
            // see the refreshed values)
            if (!rc && no_density)
                rc = asmc_pcn_flow_fused_refresh(ctx, n, prm->x_dtype == ASMC_F64 ? ASMC_F64 : ASMC_F32, lq, pd, flow, d_rho, pcn_flow_bad_cell(ctx), st);
        } else {
            rc = pcn_steps(
                loop, pd,
                [&](int, uint32_t step, int* g) -> int {
                    int r = pcn_reg_flow_launch(ctx, n, prm->x_dtype, soa ? PCN_FLOW_PROPOSE_S : PCN_FLOW_PROPOSE, x, x_prop, ll, lp, lq, ll_new,
                                                lp_new, lq_new, pd, d_rho, step, d_block, g, st);
                    if (r) return r;
                    r = asmc_coupling_logprob(ctx, n, prm->x_dtype, x_prop, flow, lq_new, stream);
                    if (r) return r;
                    return pcn_reg_flow_launch(ctx, n, prm->x_dtype, soa ? PCN_FLOW_ACCEPT_S : PCN_FLOW_ACCEPT, x, x_prop, ll, lp, lq, ll_new,
                                               lp_new, lq_new, pd, d_rho, step, d_block, g, st);
                },
                pcn_close(loop, d_block));
        }
        if (rc) return rc;
        rc = convert(PCN_UNWHITEN_X);
        if (rc) return rc;
    } else {
        // the x-state loop: the split path's kernels, one ABI step at a time
        rc = pcn_set_scalar_launch(ctx, d_rho, *rho_inout_host, st);
        if (rc) return rc;
        if (d_noise > 0) {
            asmc_set_error("asmc_pcn_mutate_flow: the zero-padded form needs the one-kernel step");
            return ASMC_ERR_UNSUPPORTED;
        }
        rc = pcn_steps(
            loop, pd,
            [&](int, uint32_t step, int* g) -> int {
                int r = pcn_propose_launch(ctx, n, d, prm->x_dtype, x, x_prop, q0, q1, pd, d_rho, step, st);
                if (r) return r;
                r = asmc_coupling_logprob(ctx, n, prm->x_dtype, x_prop, flow, lq_new, stream);
                if (r) return r;
                r = asmc_mixture_logpdf(ctx, n, d, prm->x_dtype, x_prop, &prm->log_prior, lp_new, stream);
                if (r) return r;
                r = asmc_mixture_logpdf(ctx, n, d, prm->x_dtype, x_prop, &prm->log_likelihood, ll_new, stream);
                if (r) return r;
                r = pcn_accept_flags_launch(ctx, n, ll, lp, lq, ll_new, lp_new, lq_new, nullptr, nullptr, q0, q1, prm->beta, prm->seed, prm->gid0,
                                            step, st);
                if (r) return r;
                *g = 1;  // the accept kernel's count cell plays the part of a one-block partial
                return launch_copy_flagged(ctx, n, d, prm->x_dtype, x, x_prop, ctx->d_flags, st);
            },
            pcn_close(loop, reinterpret_cast<const long long*>(ctx->d_keys)));
        if (rc) return rc;
    }
    return pcn_finish_call(ctx, n, lq, n_steps, pcn_flow_bad_cell(ctx), ctx->mutate_defer, rho_inout_host, n_accept_host, rho_hist_host, st);
}

// 32 < d <= 128 (x: the state with D = 64 / 128 columns - the problem itself or its zero-padded copy, d_noise = its real
// dimension then): whiten, n_steps launches of the one-kernel step on 16-particle groups (asmc_flow16.hip), un-whiten.  The
// carried ll / lp / lq are the step kernel's own (MM_UNWHITEN_X re-evaluates nothing).
static int pcn_mutate_flow16_impl(asmc_ctx* ctx, int64_t n, void* x, double* ll, double* lp, double* lq, const asmc_pcn_params* prm,
                                  const asmc_coupling* flow, int n_steps, uint32_t step0, double* rho_inout_host,
                                  int64_t* n_accept_host, double* rho_hist_host, asmc_stream stream, int d_noise) {
    ASMC_REQUIRE(ctx->d_mmtab != nullptr && ((uintptr_t)x % 16) == 0, "flow16: ctx was created with d_max <= 32, or a misaligned state");
    hipStream_t st = as_stream(stream);
    PcnDev pd = pcn_dev_from_params(ctx, prm, d_noise);
    pd.ll = to_dev(prm->log_likelihood);
    pd.lp = to_dev(prm->log_prior);
    pd.lq = pd.lp;  // placeholder: the proposal density is the flow
    pd.noise = prm->noise;
    double* d_rho = ctx->d_rho;
    long long* d_block = pcn_block_counts(ctx);
    unsigned long long* d_bad = pcn_flow_bad_cell(ctx);
    const PcnLoop loop = {ctx, n, prm, n_steps, step0, st};
    int rc = pcn_set_scalar_launch(ctx, d_rho, *rho_inout_host, st);
    if (rc) return rc;
    ASMC_HIP(hipMemsetAsync(d_bad, 0, sizeof(unsigned long long), st));
    rc = asmc_pcn_mm_pack(ctx, pd, st);
    if (rc) return rc;
    rc = asmc_pcn_flow16_tables(ctx, pd, flow, st);
    if (rc) return rc;
    int grid = 0;
    rc = asmc_pcn_mm_launch(ctx, n, prm->x_dtype, x, ll, lp, lq, pd, MM_WHITEN, d_rho, 0, d_block, &grid, st);
    if (rc) return rc;
    rc = pcn_steps(
        loop, pd,
        [&](int, uint32_t step, int* g) { return asmc_pcn_flow16_launch(ctx, n, prm->x_dtype, x, ll, lp, lq, pd, flow, d_rho, step, d_block, g, d_bad, st); },
        pcn_close(loop, d_block));
    if (rc) return rc;
    rc = asmc_pcn_mm_launch(ctx, n, prm->x_dtype, x, ll, lp, lq, pd, MM_UNWHITEN_X, d_rho, 0, d_block, &grid, st);
    if (rc) return rc;
    return pcn_finish_call(ctx, n, lq, n_steps, d_bad, ctx->mutate_defer, rho_inout_host, n_accept_host, rho_hist_host, st);
}

// The tail of a flow mutation on a zero-padded copy xp of the state x.  The un-padding copy must sit behind the mutation on the
// stream AND in front of the read-back's synchronisation: the blocking form returns with x final (it used to synchronise
// inside the implementation and enqueue the copy after that, so a C caller reading x on another stream saw the padded run's
// input).  So the implementation always runs deferred here, the copy follows, and the blocking form collects afterwards.
template <typename Impl>
static int pcn_flow_padded_tail(asmc_ctx* ctx, int64_t n, int d, int D, int x_dtype, const void* xp, void* x, int n_steps,
                                double* rho_inout_host, int64_t* n_accept_host, double* rho_hist_host, hipStream_t st, Impl impl) {
    const int caller_defers = ctx->mutate_defer;
    ctx->mutate_defer = 1;
    int rc = impl();
    ctx->mutate_defer = caller_defers;
    if (rc) return rc;
    rc = launch_unpad_rows(ctx, n, d, D, x_dtype, xp, x, st);
    if (rc) return rc;
    if (caller_defers) return ASMC_OK;  // asmc_pcn_mutate_flow_result waits for the mutation's event; the copy is stream-ordered behind it
    ctx->mutate_pending_steps = 0;
    // (stream synchronisation, not the event recorded in front of the copy: x must be final when this call returns)
    return pcn_collect(ctx, n_steps, true, true, rho_inout_host, n_accept_host, rho_hist_host, st);
}

extern "C" {

int asmc_pcn_mutate_flow(asmc_ctx* ctx, int64_t n, void* x, double* ll, double* lp, double* lq,
                         const asmc_pcn_params* prm, const asmc_coupling* flow, void* work_dev, int64_t work_bytes,
                         int n_steps, uint32_t step0, double* rho_inout_host, int64_t* n_accept_host,
                         double* rho_hist_host, asmc_stream stream) {
    ASMC_REQUIRE(ctx && x && prm && flow, "null pointer");  // (what choosing the path below reads; the call's check follows it)
    if (ctx->chain_on) {  // (an MCMC target has no proposal-density term: nothing to record from the flow-proposal step)
        asmc_set_error("asmc_pcn_mutate_flow: the chain recorder is honoured by asmc_pcn_mutate only (asmc_chain_clear first)");
        return ASMC_ERR_UNSUPPORTED;
    }
    ASMC_REQUIRE(flow->affine == ASMC_AFFINE_TANH || (flow->affine == ASMC_AFFINE_SOFTCLIP && flow->kind == ASMC_FLOW_MAF),
                 "bad affine form (the soft-clipped form is for autoregressive flows)");
    // Fewer than 32 dimensions: the one-kernel step on a zero-padded copy (pcn_mutate_padded's scheme: padded rows and tables,
    // the identity beyond d, no noise there) wherever the flow's shape is one the kernel takes - any even d for a coupling flow,
    // any d for an autoregressive one.  Round 3 ran propose / flow / accept kernels at d = 8 / 16 (0.35 / 0.42 ms per step
    // at 1M particles) and the x-state split path at the other d (0.8 ms at d = 20).
    // More than 32 dimensions (round 5): the one-kernel step on 16-particle groups at D = 64 / 128 (asmc_flow16.hip), the
    // problem zero-padded to D when it is narrower.  Round 4 ran propose / flow / targets / accept / copy kernels at 32 < d <= 64
    // with a coupling flow (1.2 - 1.8 ms per step at 1M particles) and had no device path for an autoregressive flow there.
    // (... and at d <= 32 when the flow itself lives in that layout: asmc_flow_layout = 1, an autoregressive flow of hidden width 128)
    const int d = prm->d;
    const bool lay16 = asmc_flow_layout(flow->kind, flow->dims, flow->hidden) == 1;
    int D16 = 0;  // the width of the 16-particle-group step, where it serves the call
    asmc_pcn_params p16 = *prm;
    if ((d > 32 || lay16) && d <= 128 && d == flow->dims && ctx->d_mmtab && !pcn_env_generic() && !pcn_env_nopad() && !pcn_env_xstate()) {
        const int D = d <= 64 ? 64 : 128;
        p16.d = D;
        if ((D <= ctx->d_max_pad || d <= 32) && asmc_pcn_flow16_ok(&p16, flow)) D16 = D;
    }
    asmc_pcn_params p2 = *prm;
    p2.d = 32;
    const bool pad32 = !D16 && d >= 2 && d < 32 && d == flow->dims && 32 <= ctx->d_max_pad && !pcn_env_generic() && !pcn_env_nopad() &&
                       asmc_pcn_flow_fused_ok(&p2, flow) && !pcn_env_aos() && !pcn_env_xstate();
    // What the serving path requires: the 16-particle-group step takes no work buffer; the x-state loop never reads the noise mode.
    const bool reads_noise = D16 || pad32 || (pcn_reg_supported(d, prm->x_dtype == ASMC_F64 ? 8 : 4, x) && !pcn_env_xstate());
    int rc = pcn_check_call(__func__, ctx, n, x, ll, lp, lq, prm, n_steps, rho_inout_host, n_accept_host,
                            {2, reads_noise, flow, !D16, work_dev, work_bytes});
    if (rc) return rc;
    hipStream_t st = as_stream(stream);
    if (D16) {
        if (d == D16 && ((uintptr_t)x % 16) == 0)
            return pcn_mutate_flow16_impl(ctx, n, x, ll, lp, lq, prm, flow, n_steps, step0, rho_inout_host, n_accept_host, rho_hist_host,
                                          stream, 0);
        void* xp = nullptr;
        rc = pcn_pad_params(ctx, n, x, prm, D16, 2, st, &p16, &xp);
        if (rc) return rc;
        return pcn_flow_padded_tail(ctx, n, d, D16, prm->x_dtype, xp, x, n_steps, rho_inout_host, n_accept_host, rho_hist_host, st, [&]() {
            return pcn_mutate_flow16_impl(ctx, n, xp, ll, lp, lq, &p16, flow, n_steps, step0, rho_inout_host, n_accept_host,
                                          rho_hist_host, stream, d);
        });
    }
    if (pad32) {
        void* xp = nullptr;
        rc = pcn_pad_params(ctx, n, x, prm, 32, 2, st, &p2, &xp);
        if (rc) return rc;
        rc = pcn_flow_padded_tail(ctx, n, d, 32, prm->x_dtype, xp, x, n_steps, rho_inout_host, n_accept_host, rho_hist_host, st, [&]() {
            return pcn_mutate_flow_impl(ctx, n, xp, ll, lp, lq, &p2, flow, work_dev, n_steps, step0, rho_inout_host, n_accept_host,
                                        rho_hist_host, stream, d);
        });
        if (rc != ASMC_ERR_UNSUPPORTED) return rc;
        // the one-kernel step declined after the pre-check (no register path for this pointer, no coordinate-major state): nothing
        // of the caller's has been touched yet (only the padded copy was whitened) - the unpadded path serves the shape, as before
        // (only the implementation answers this code: the tail's own launches and copies fail with ASMC_ERR_HIP)
        ctx->mutate_pending_steps = 0;
    }
    return pcn_mutate_flow_impl(ctx, n, x, ll, lp, lq, prm, flow, work_dev, n_steps, step0, rho_inout_host, n_accept_host, rho_hist_host,
                                stream, 0);
}

int asmc_pcn_mutate_flow_enqueue(asmc_ctx* ctx, int64_t n, void* x, double* ll, double* lp, double* lq,
                                 const asmc_pcn_params* prm, const asmc_coupling* flow, void* work_dev, int64_t work_bytes,
                                 int n_steps, uint32_t step0, double rho, asmc_stream stream) {
    ASMC_REQUIRE(ctx != nullptr, "null ctx");
    ASMC_REQUIRE(ctx->mutate_pending_steps == 0, "a deferred mutation is still pending (asmc_pcn_mutate_flow_result)");
    int64_t dummy_acc = 0;
    ctx->mutate_defer = 1;
    const int rc = asmc_pcn_mutate_flow(ctx, n, x, ll, lp, lq, prm, flow, work_dev, work_bytes, n_steps, step0, &rho, &dummy_acc,
                                        nullptr, stream);
    ctx->mutate_defer = 0;
    return rc;
}

int asmc_pcn_mutate_flow_result(asmc_ctx* ctx, int n_steps, double* rho_out_host, int64_t* n_accept_host, double* rho_hist_host,
                                asmc_stream stream) {
    ASMC_REQUIRE(ctx && rho_out_host && n_accept_host, "null pointer");
    ASMC_REQUIRE(ctx->mutate_pending_steps == n_steps && n_steps > 0, "no deferred mutation of this length is pending");
    ctx->mutate_pending_steps = 0;
    return pcn_collect(ctx, n_steps, true, true, rho_out_host, n_accept_host, rho_hist_host, as_stream(stream), ctx->ev_mutate);
}

int64_t asmc_pcn_flow_nonfinite(asmc_ctx* ctx) { return ctx ? (int64_t)ctx->flow_nonfinite : -1; }

int64_t asmc_pcn_lq_nan(asmc_ctx* ctx) { return ctx ? (int64_t)ctx->lq_nan : -1; }

// ==== the accept-count exchange of sharded runs: the count hook, and RCCL on the step kernels' own stream ===================
int asmc_pcn_set_count_hook(asmc_ctx* ctx, asmc_count_hook hook, void* user, int64_t* cell_dev, int64_t n_global) {
    ASMC_REQUIRE(ctx != nullptr, "null ctx");
    ASMC_REQUIRE(hook == nullptr || (cell_dev != nullptr && n_global > 0), "hook needs a device cell and n_global > 0");
    ctx->count_hook = hook;
    ctx->count_hook_user = user;
    ctx->count_cell = reinterpret_cast<long long*>(cell_dev);
    ctx->count_n_global = n_global;
    ctx->count_cells = 1;  // (asmc_pcn_set_count_cells widens it)
    return ASMC_OK;
}

int asmc_pcn_set_count_cells(asmc_ctx* ctx, int n_cells) {
    ASMC_REQUIRE(ctx != nullptr && n_cells >= 1 && n_cells <= ASMC_MAX_COUNT_CELLS, "n_cells out of range");
    ctx->count_cells = n_cells;
    return ASMC_OK;
}

// the exchange issued by the library: RCCL's all-reduce on the step kernels' own stream (include/asmc.h)
typedef int (*rccl_allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
static int rccl_count_hook(void* user, asmc_stream stream) {
    asmc_ctx* ctx = static_cast<asmc_ctx*>(user);
    const int nccl_int64 = 4, nccl_sum = 0;  // rccl.h: ncclInt64, ncclSum
    return reinterpret_cast<rccl_allreduce_fn>(ctx->rccl_allreduce)(ctx->count_cell, ctx->count_cell, (size_t)ctx->count_cells, nccl_int64, nccl_sum,
                                                                    ctx->rccl_comm, reinterpret_cast<hipStream_t>(stream));
}

int asmc_set_rccl(asmc_ctx* ctx, void* allreduce_fn, void* nccl_comm) {
    ASMC_REQUIRE(ctx != nullptr, "null ctx");
    ASMC_REQUIRE((allreduce_fn == nullptr) == (nccl_comm == nullptr), "function and communicator come together");
    ctx->rccl_allreduce = allreduce_fn;
    ctx->rccl_comm = nccl_comm;
    return ASMC_OK;
}

int asmc_set_rccl_allgather(asmc_ctx* ctx, void* allgather_fn) {
    ASMC_REQUIRE(ctx != nullptr, "null ctx");
    ctx->rccl_allgather = allgather_fn;
    return ASMC_OK;
}

// equal-sized all-gather of 8-byte elements on the library's communicator and stream (the small exchanges of owner-layout
// resampling: evidence partials, chain states, kept counts)
int asmc_rccl_all_gather(asmc_ctx* ctx, const void* send_dev, void* recv_dev, int64_t count, int is_int64, asmc_stream stream) {
    ASMC_REQUIRE(ctx && send_dev && recv_dev && count > 0, "bad arguments");
    ASMC_REQUIRE(ctx->rccl_allgather && ctx->rccl_comm, "asmc_set_rccl / asmc_set_rccl_allgather first");
    typedef int (*allgather_fn)(const void*, void*, size_t, int, void*, hipStream_t);
    const int dt = is_int64 ? 4 : 8;  // rccl.h: ncclInt64, ncclFloat64
    if (reinterpret_cast<allgather_fn>(ctx->rccl_allgather)(send_dev, recv_dev, (size_t)count, dt, ctx->rccl_comm,
                                                            reinterpret_cast<hipStream_t>(stream)) != 0) {
        asmc_set_error("asmc_rccl_all_gather: ncclAllGather failed");
        return ASMC_ERR_ARG;
    }
    return ASMC_OK;
}

int asmc_pcn_set_count_rccl(asmc_ctx* ctx, int64_t* cell_dev, int64_t n_global) {
    ASMC_REQUIRE(ctx != nullptr, "null ctx");
    if (cell_dev == nullptr) return asmc_pcn_set_count_hook(ctx, nullptr, nullptr, nullptr, 0);
    ASMC_REQUIRE(ctx->rccl_allreduce && ctx->rccl_comm, "asmc_set_rccl first");
    return asmc_pcn_set_count_hook(ctx, rccl_count_hook, ctx, cell_dev, n_global);
}

}  // extern "C"
