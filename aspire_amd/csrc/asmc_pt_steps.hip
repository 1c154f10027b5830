// asmc_pt_steps.hip - the rung-batched step loop and the adaptive ladder of the "pt_minipcn" sampler (include/asmc.h, ABI 30;
// DESIGN.md §3.22): every launch of a Markov step covers all T rungs of the tempered ensemble, and everything that differs between
// the rungs - beta, the reference's tables, nu, the step size, the accept count - lives in device tables indexed by the rung.
//
// The step itself is pcn_reg_body (asmc_pcn_reg.h), unchanged: k_pt_reg forms rung blockIdx.y's view of the state and calls it,
// so a rung's step is, bit for bit, the x-state step asmc_pcn_mutate runs on that rung's rows.  The kernels around it are the
// per-rung forms of k_pcn_pack, k_gamma_draw, k_pcn_adapt and k_chain_rows.  Every index is 64-bit.
#include "asmc_pcn_reg.h"

// ---- the step -------------------------------------------------------------------------------------------------------------------
// grid (ceil(W / (64 wpb)), T).  What the rungs share arrives as k_pcn_reg's by-value PcnScalars `shared`; what they do not, as tables
// indexed by r = blockIdx.y: betas [T], nus [T] (> 0: a Student-t reference, else Gaussian), the table blocks `stride` doubles
// apart, rho [T], shared.gam [T W].  The rung's scalars are reads of `const __restrict__` kernel arguments at an index formed from
// blockIdx.y alone: wave-uniform, scalar loads (§3.10: none of them steers a branch inside the body - beta and nu enter arithmetic
// only, and the component counts, which do, are kernel arguments as in k_pcn_reg).  The tables must be kernel arguments of their
// own: as pointers inside a by-value struct they lose `noalias`, and the d = 32 instantiations then held 120 more scalar registers
// in vector lanes, took 60 more vector registers and spilled (§3.22).  The reference's kind is the compile-time MODE, as in
// k_pcn_reg; a tpCN fit may hand single rungs a Gaussian reference (nu above NU_GAUSSIAN), and then both instantiations are launched
// over the same grid and a block whose rung is of the other kind leaves at once, before any barrier.
template <typename T, int D, int MODE>
__global__ __launch_bounds__(ASMC_BLOCK, 2) void k_pt_reg(int64_t W, T* __restrict__ x, double* __restrict__ ll, double* __restrict__ lp,
                                                         double* __restrict__ lq, const double* __restrict__ ptab, PcnScalars shared,
                                                         const double* __restrict__ betas, const double* __restrict__ nus, int stride,
                                                         const double* __restrict__ rho, uint32_t step,
                                                         long long* __restrict__ block_counts) {
    constexpr bool TP = MODE == PCN_X_STEP_T;
    const int r = (int)blockIdx.y;
    const int64_t row0 = (int64_t)r * W;
    const double nu = nus[r];
    if ((nu > 0.0) != TP) return;
    PcnScalars p = shared;
    p.beta = betas[r];
    p.nu = nu;
    p.gam = TP ? shared.gam + row0 : nullptr;
    p.gid0 = (unsigned long long)row0;
    pcn_reg_body<T, D, ASMC_NOISE_F64, MODE>(W, x + row0 * D, ll + row0, lp + row0, lq + row0, ptab + (size_t)r * (size_t)stride, p, rho + r, step,
                                             block_counts + (size_t)r * gridDim.x);
}

// ---- the launches around it -----------------------------------------------------------------------------------------------------
struct PtPackArgs {
    const double* mu[ASMC_PT_MAX_RUNGS];
    const double* L[ASMC_PT_MAX_RUNGS];
    const double* Linv[ASMC_PT_MAX_RUNGS];
    double nu[ASMC_PT_MAX_RUNGS];
    MixDev ll, lp, lq;
    int d, stride;
};

// block r: rung r's table block (k_pcn_pack's gather) and its nu
__global__ __launch_bounds__(256) void k_pt_pack(PtPackArgs a, double* __restrict__ tab, double* __restrict__ nu_out) {
    const int r = (int)blockIdx.x;
    PcnDev pd;
    pd.d = a.d;
    pd.dpad = 0;
    pd.mu = a.mu[r];
    pd.L = a.L[r];
    pd.Linv = a.Linv[r];
    pd.ll = a.ll;
    pd.lp = a.lp;
    pd.lq = a.lq;
    pcn_pack_block(pd, tab + (size_t)r * (size_t)a.stride);
    if (threadIdx.x == 0) nu_out[r] = a.nu[r];
}

// k_gamma_draw over all rungs: walker i = r W + w draws Gamma((d + nu_r) / 2) at gid = i for the steps step .. step + nsteps - 1
// (rungs with a Gaussian reference draw nothing)
__global__ __launch_bounds__(ASMC_BLOCK) void k_pt_gamma(int64_t n, int64_t W, int d, const double* __restrict__ nu, unsigned long long seed,
                                                        uint32_t step, int nsteps, int64_t stride_n, double* __restrict__ out,
                                                        const double* __restrict__ bmtab) {
    bm_d2* bmt = bm_lds();
    bm_tab_stage<ASMC_BLOCK>(bmt, bmtab);
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * ASMC_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x; i < n; i += stride) {
        const double nu_r = nu[i / W];
        if (!(nu_r > 0.0)) continue;
        const double shape = 0.5 * ((double)d + nu_r);
        for (int s = 0; s < nsteps; s++)
            out[(size_t)s * stride_n + i] = gamma_unit<false>(shape, seed, (unsigned long long)i, step + (uint32_t)s, bmt);
    }
}

// block r closes rung r's step: k_pcn_adapt's sum and update with the rung's own cells
__global__ __launch_bounds__(256) void k_pt_close(int nblocks, const long long* __restrict__ block_counts, int64_t W, int t,
                                                 long long* __restrict__ accept, double* __restrict__ rho, double target, int adapt) {
    __shared__ long long s_c[4];
    const int r = (int)blockIdx.x;
    const long long* __restrict__ bc = block_counts + (size_t)r * (size_t)nblocks;
    long long c = 0;
    for (int b = threadIdx.x; b < nblocks; b += 256) c += bc[b];
    c = wave_sum_ll(c);
    if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        c = s_c[0] + s_c[1] + s_c[2] + s_c[3];
        accept[r] += c;
        if (adapt) rho[r] = pcn_adapt_rho(rho[r], c, W, target, t);
    }
}

// k_chain_rows over all rungs: the state [T W] rows of `units` -> slot `slot` of every rung in a chain [T, S, W]; rung r's rows
// stay together, (r (S - 1) + slot) W rows further on
template <typename V>
__global__ __launch_bounds__(ASMC_BLOCK) void k_pt_chain_rows(int64_t n, int64_t W, int64_t units, int64_t S, int64_t slot,
                                                             const V* __restrict__ src, V* __restrict__ dst, const double* __restrict__ ll,
                                                             const double* __restrict__ lp, double* __restrict__ ll_out,
                                                             double* __restrict__ lp_out) {
    const int64_t stride = (int64_t)gridDim.x * ASMC_BLOCK;
    const int64_t i0 = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x;
    const int64_t total = n * units, rung = W * units;
    for (int64_t e = i0; e < total; e += stride) dst[e + ((e / rung) * (S - 1) + slot) * rung] = src[e];
    for (int64_t i = i0; i < n; i += stride) {
        const int64_t o = i + ((i / W) * (S - 1) + slot) * W;
        ll_out[o] = ll[i];
        lp_out[o] = lp[i];
    }
}

// the ladder update: one block, fp64.  Lanes form the pairs' acceptances, lane 0 the gaps and their running sum (T <= 64 terms, in
// index order), lanes write the history row.
__global__ __launch_bounds__(ASMC_WAVE) void k_pt_ladder(int T, int64_t W, const long long* __restrict__ counts, long long* __restrict__ snap,
                                                        double* __restrict__ betas, double* __restrict__ hist, double kappa) {
    __shared__ double s_a[ASMC_PT_MAX_RUNGS];
    const int i = (int)threadIdx.x;
    if (i < T - 1) {
        const long long c = counts[i];
        s_a[i] = (double)(c - snap[i]) / (double)W;
        snap[i] = c;
    }
    __syncthreads();
    if (i == 0) {
        double inv_prev = 1.0 / betas[0], sum = 1.0;
        for (int k = 1; k <= T - 2; k++) {
            const double inv = 1.0 / betas[k];
            const double g = (inv - inv_prev) * exp(kappa * (s_a[k - 1] - s_a[k]));
            inv_prev = inv;
            sum += g;
            betas[k] = 1.0 / sum;
        }
    }
    __syncthreads();
    if (i < T) hist[i] = betas[i];
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
#define PT_UNSUPPORTED(cond, ...)           \
    do {                                    \
        if (cond) {                         \
            asmc_set_error(__VA_ARGS__);    \
            return ASMC_ERR_UNSUPPORTED;    \
        }                                   \
    } while (0)

static constexpr int PT_WPB = 4;  // launch_pcn_reg's rule for a kernel that draws the default noise: four waves share its tables
static int pt_table_stride(int d) { return 2 * (d * (d + 1) / 2) + d + 3 * ASMC_MAX_COMPONENTS * (1 + 2 * d) + (d / 4) * (d / 4 + 1) / 2 * 16; }
static int64_t pt_grid_x(int64_t W) { return ((W + 63) / 64 + PT_WPB - 1) / PT_WPB; }
// d_pt: tables [T stride] | nu [ASMC_PT_MAX_RUNGS] | block counts [T grid]
static double* pt_nu(const asmc_ctx* ctx) { return ctx->d_pt + (size_t)ctx->pt_T * pt_table_stride(ctx->pt_d); }
static long long* pt_block_counts(const asmc_ctx* ctx) { return reinterpret_cast<long long*>(pt_nu(ctx) + ASMC_PT_MAX_RUNGS); }

static int pt_scope(const char* fn, const asmc_pcn_params* prm, const void* x) {
    PT_UNSUPPORTED(prm->noise != ASMC_NOISE_F64, "%s: the rung-batched step draws the default fp64 noise only", fn);
    PT_UNSUPPORTED(!(prm->d == 4 || prm->d == 8 || prm->d == 16 || prm->d == 32),
                   "%s: d=%d is not a register-kernel width (4, 8, 16, 32); the zero-padded form is not batched", fn, prm->d);
    PT_UNSUPPORTED(x != nullptr && !pcn_reg_supported(prm->d, prm->x_dtype == ASMC_F64 ? 8 : 4, x),
                   "%s: the state is not 16-byte aligned, or the register kernels are switched off (ASMC_PCN_GENERIC)", fn);
    PT_UNSUPPORTED(prm->adapt != 0 && prm->adapt != 1, "%s: a lagged adaptation (adapt=%d) is not batched", fn, prm->adapt);
    return ASMC_OK;
}

template <typename T, int D, int MODE>
static int launch_pt_reg(asmc_ctx* ctx, int n_temps, int64_t W, T* x, double* ll, double* lp, double* lq, const PcnScalars& a,
                         const double* betas, const double* rho, uint32_t step, hipStream_t st) {
    constexpr size_t lds_bytes = (size_t)PT_WPB * 64 * (D * sizeof(T) + 16);
    auto kern = k_pt_reg<T, D, MODE>;
    static bool attr_set_dev[ASMC_MAX_DEVICES] = {false};
    bool& attr_set = attr_set_dev[asmc_dev_slot(ctx)];
    if (lds_bytes > 64 * 1024 && !attr_set) {  // (d = 32 fp64: four tiles are 69 632 bytes)
        ASMC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        attr_set = true;
    }
    ASMC_LAUNCH(ctx, st, MODE == PCN_X_STEP_T ? "k_tpt_reg" : "k_pt_reg", kern, dim3((unsigned)ctx->pt_grid, (unsigned)n_temps),
                dim3(PT_WPB * 64), lds_bytes, st, W, x, ll, lp, lq, (const double*)ctx->d_pt, a, betas, (const double*)pt_nu(ctx), pt_table_stride(D), rho, step,
                pt_block_counts(ctx));
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

// `tp`: the instantiation for the rungs with a Student-t reference, else the one for the Gaussian rungs
template <typename T>
static int dispatch_pt_reg(asmc_ctx* ctx, int n_temps, int64_t W, int d, bool tp, void* x, double* ll, double* lp, double* lq,
                           const PcnScalars& a, const double* betas, const double* rho, uint32_t step, hipStream_t st) {
#define PT_CASE(DD)                                                                                                         \
    case DD:                                                                                                                \
        return tp ? launch_pt_reg<T, DD, PCN_X_STEP_T>(ctx, n_temps, W, static_cast<T*>(x), ll, lp, lq, a, betas, rho, step, st)   \
                  : launch_pt_reg<T, DD, PCN_X_STEP>(ctx, n_temps, W, static_cast<T*>(x), ll, lp, lq, a, betas, rho, step, st);
    switch (d) {
        PT_CASE(4)
        PT_CASE(8)
        PT_CASE(16)
        PT_CASE(32)
    }
#undef PT_CASE
    asmc_set_error("asmc_pt_steps: no kernel for d=%d", d);
    return ASMC_ERR_UNSUPPORTED;
}

extern "C" {

int asmc_pt_steps_supported(int d, int x_dtype, const void* x) {
    return (x_dtype == ASMC_F64 || x_dtype == ASMC_F32) && x != nullptr && pcn_reg_supported(d, x_dtype == ASMC_F64 ? 8 : 4, x) ? 1 : 0;
}

int asmc_pt_pack(asmc_ctx* ctx, int T, int64_t W, const asmc_pcn_params* prm, const double* const* mu, const double* const* L,
                 const double* const* Linv, const double* nu_host, asmc_stream stream) {
    ASMC_REQUIRE(ctx != nullptr && prm != nullptr && mu != nullptr && L != nullptr && Linv != nullptr, "null pointer");
    ASMC_REQUIRE(T >= 1 && T <= ASMC_PT_MAX_RUNGS, "n_temps outside 1 .. ASMC_PT_MAX_RUNGS");
    ASMC_REQUIRE(W > 0 && W <= ctx->n_max / T, "n_temps * n_walkers out of range for this ctx");
    ASMC_REQUIRE(prm->x_dtype == ASMC_F64 || prm->x_dtype == ASMC_F32, "bad x_dtype");
    int rc = pt_scope(__func__, prm, nullptr);
    if (!rc) rc = check_mixture(prm->log_likelihood);
    if (!rc) rc = check_mixture(prm->log_prior);
    if (!rc) rc = check_mixture(prm->log_q);
    if (rc) return rc;
    int kinds = 0;  // 1: some rung has a Gaussian reference, 2: some rung a Student-t one
    PtPackArgs a;
    memset(&a, 0, sizeof(a));
    for (int r = 0; r < T; r++) {
        ASMC_REQUIRE(mu[r] && L[r] && Linv[r], "null reference pointer of a rung");
        const double nu = nu_host ? nu_host[r] : 0.0;
        ASMC_REQUIRE(!(nu > 0.0) || nu >= 1.0, "a rung's nu must be >= 1 (or <= 0 for the Gaussian reference)");
        kinds |= nu > 0.0 ? 2 : 1;
        a.mu[r] = mu[r];
        a.L[r] = L[r];
        a.Linv[r] = Linv[r];
        a.nu[r] = nu > 0.0 ? nu : 0.0;
    }
    a.ll = to_dev(prm->log_likelihood);
    a.lp = to_dev(prm->log_prior);
    a.lq = to_dev(prm->log_q);
    a.d = prm->d;
    a.stride = pt_table_stride(prm->d);
    const int64_t grid = pt_grid_x(W);
    PT_UNSUPPORTED(grid > ASMC_PCN_MAX_GRID, "asmc_pt_pack: n_walkers=%lld exceeds the per-launch block budget", (long long)W);
    const size_t need = sizeof(double) * ((size_t)T * (size_t)a.stride + ASMC_PT_MAX_RUNGS) + sizeof(long long) * (size_t)T * (size_t)grid;
    if (need > ctx->pt_bytes) {
        ASMC_HIP(hipDeviceSynchronize());  // (steps of an earlier pack may still read the old tables)
        if (ctx->d_pt) (void)hipFree(ctx->d_pt);
        ctx->d_pt = nullptr;
        ctx->pt_bytes = 0;
        ctx->pt_T = 0;
        if (hipMalloc(reinterpret_cast<void**>(&ctx->d_pt), need) != hipSuccess) {
            (void)hipGetLastError();
            asmc_set_error("asmc_pt_pack: no device memory for %zu bytes of rung tables", need);
            return ASMC_ERR_NOMEM;
        }
        ctx->pt_bytes = need;
    }
    ctx->pt_T = T, ctx->pt_d = prm->d, ctx->pt_tp = kinds, ctx->pt_W = W, ctx->pt_grid = (int)grid;
    ctx->pt_c[0] = a.ll.C, ctx->pt_c[1] = a.lp.C, ctx->pt_c[2] = a.lq.C;
    hipStream_t st = as_stream(stream);
    ASMC_LAUNCH(ctx, st, "k_pt_pack", k_pt_pack, dim3(T), dim3(256), 0, st, a, ctx->d_pt, pt_nu(ctx));
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int asmc_pt_steps(asmc_ctx* ctx, int T, int64_t W, void* x, double* ll, double* lp, double* lq, const asmc_pcn_params* prm,
                  const double* betas, double* rho, int64_t* accept, int n_steps, uint32_t step0, const asmc_chain_target* ch,
                  int64_t slot0, asmc_stream stream) {
    ASMC_REQUIRE(ctx && x && ll && lp && lq && prm && betas && rho && accept, "null pointer");
    ASMC_REQUIRE(T >= 1 && T <= ASMC_PT_MAX_RUNGS, "n_temps outside 1 .. ASMC_PT_MAX_RUNGS");
    ASMC_REQUIRE(W > 0 && W <= ctx->n_max / T, "n_temps * n_walkers out of range for this ctx");
    ASMC_REQUIRE(n_steps >= 1 && n_steps <= ASMC_MAX_PCN_STEPS, "n_steps out of range (<= 2048 per call)");
    ASMC_REQUIRE(prm->x_dtype == ASMC_F64 || prm->x_dtype == ASMC_F32, "bad x_dtype");
    int rc = pt_scope(__func__, prm, x);
    if (rc) return rc;
    PT_UNSUPPORTED(ctx->count_hook != nullptr, "asmc_pt_steps: a sharded run (accept-count exchange installed) is not batched");
    ASMC_REQUIRE(ctx->d_pt != nullptr && ctx->pt_T == T && ctx->pt_W == W && ctx->pt_d == prm->d, "no asmc_pt_pack of this n_temps, n_walkers and d");
    const bool tp = (ctx->pt_tp & 2) != 0;
    const int64_t n = (int64_t)T * W;
    if (ch != nullptr) {
        ASMC_REQUIRE(ch->x_dev && ch->ll_dev && ch->lp_dev, "chain: null pointer");
        ASMC_REQUIRE(ch->n == W && ch->d == prm->d && ch->pitch == prm->d && ch->x_dtype == prm->x_dtype, "chain: n, d, pitch or dtype differ from the call's");
        ASMC_REQUIRE(slot0 >= 0 && ch->n_slots > 0 && slot0 + n_steps <= ch->n_slots, "chain: the call's steps do not fit a rung's slots");
    }
    hipStream_t st = as_stream(stream);
    PcnScalars a;  // what the rungs share; beta, nu, gid0 and the variates' offset are the kernel's to fill
    memset(&a, 0, sizeof(a));
    a.d_real = prm->d;
    a.bmtab = ctx->d_bmtab;
    a.seed = prm->seed;
    a.c_ll = ctx->pt_c[0], a.c_lp = ctx->pt_c[1], a.c_lq = ctx->pt_c[2];
    const size_t elem = prm->x_dtype == ASMC_F64 ? 8 : 4, rowb = (size_t)prm->d * elem;
    const int64_t gam_stride = (n + 63) / 64 * 64;  // (<= n_max + 63: ASMC_GAMMA_BATCH steps fit ctx->d_gamma)
    ctx->gam_count = 0;  // the variates below are not a batch pcn_prepare_gamma knows: a later per-rung call draws its own
    int gam_have = 0, gam_t0 = 0;
    for (int t = 0; t < n_steps; t++) {
        const uint32_t step = step0 + (uint32_t)t;
        if (tp) {
            if (t - gam_t0 >= gam_have) {
                gam_t0 = t;
                gam_have = n_steps - t < ASMC_GAMMA_BATCH ? n_steps - t : ASMC_GAMMA_BATCH;
                ASMC_LAUNCH(ctx, st, "k_pt_gamma", k_pt_gamma, dim3(grid_for(n, ASMC_BLOCK, ASMC_MAX_BLOCKS * 4)), dim3(ASMC_BLOCK), 0, st, n, W,
                            prm->d, (const double*)pt_nu(ctx), (unsigned long long)prm->seed, step, gam_have, gam_stride, ctx->d_gamma,
                            (const double*)ctx->d_bmtab);
                ASMC_LAUNCH_CHECK();
            }
            a.gam = ctx->d_gamma + (size_t)(t - gam_t0) * (size_t)gam_stride;
        }
        for (int kind = 1; kind <= 2; kind <<= 1) {  // one launch; two where the rungs' references are of both kinds
            if (!(ctx->pt_tp & kind)) continue;
            rc = prm->x_dtype == ASMC_F64 ? dispatch_pt_reg<double>(ctx, T, W, prm->d, kind == 2, x, ll, lp, lq, a, betas, rho, step, st)
                                          : dispatch_pt_reg<float>(ctx, T, W, prm->d, kind == 2, x, ll, lp, lq, a, betas, rho, step, st);
            if (rc) return rc;
        }
        ASMC_LAUNCH(ctx, st, "k_pt_close", k_pt_close, dim3(T), dim3(256), 0, st, ctx->pt_grid, (const long long*)pt_block_counts(ctx), W, t,
                    reinterpret_cast<long long*>(accept), rho, prm->target_accept, prm->adapt);
        ASMC_LAUNCH_CHECK();
        if (ch != nullptr) {
            const bool vec = rowb % 16 == 0 && ((uintptr_t)x | (uintptr_t)ch->x_dev) % 16 == 0;
            const int64_t units = vec ? (int64_t)(rowb / 16) : prm->d;
            const int grid = grid_for(n * units, ASMC_BLOCK, 8192);
            const int64_t slot = slot0 + t;
            if (vec)
                ASMC_LAUNCH(ctx, st, "k_pt_chain_rows", k_pt_chain_rows<uint4>, dim3(grid), dim3(ASMC_BLOCK), 0, st, n, W, units, ch->n_slots, slot,
                            (const uint4*)x, (uint4*)ch->x_dev, (const double*)ll, (const double*)lp, ch->ll_dev, ch->lp_dev);
            else if (elem == 8)
                ASMC_LAUNCH(ctx, st, "k_pt_chain_rows", k_pt_chain_rows<double>, dim3(grid), dim3(ASMC_BLOCK), 0, st, n, W, units, ch->n_slots, slot,
                            (const double*)x, (double*)ch->x_dev, (const double*)ll, (const double*)lp, ch->ll_dev, ch->lp_dev);
            else
                ASMC_LAUNCH(ctx, st, "k_pt_chain_rows", k_pt_chain_rows<float>, dim3(grid), dim3(ASMC_BLOCK), 0, st, n, W, units, ch->n_slots, slot,
                            (const float*)x, (float*)ch->x_dev, (const double*)ll, (const double*)lp, ch->ll_dev, ch->lp_dev);
            ASMC_LAUNCH_CHECK();
        }
    }
    return ASMC_OK;
}

int asmc_pt_ladder_adapt(asmc_ctx* ctx, int T, int64_t W, const int64_t* counts, int64_t* snap, double* betas, double* hist, int update,
                         double lag, double time, asmc_stream stream) {
    ASMC_REQUIRE(ctx && counts && snap && betas && hist, "null pointer");
    ASMC_REQUIRE(T >= 3 && T <= ASMC_PT_MAX_RUNGS, "n_temps outside 3 .. ASMC_PT_MAX_RUNGS");
    ASMC_REQUIRE(W > 0 && update >= 1 && lag > 0.0 && time > 0.0, "bad n_walkers / update number / lag / time");
    hipStream_t st = as_stream(stream);
    const double kappa = lag / (time * ((double)(update - 1) + lag));
    ASMC_LAUNCH(ctx, st, "k_pt_ladder", k_pt_ladder, dim3(1), dim3(ASMC_WAVE), 0, st, T, W, reinterpret_cast<const long long*>(counts),
                reinterpret_cast<long long*>(snap), betas, hist + (size_t)update * (size_t)T, kappa);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

}  // extern "C"
