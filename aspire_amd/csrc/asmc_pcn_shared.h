// asmc_pcn_shared.h — what more than one of asmc_pcn.hip, asmc_pcn_drive.hip, asmc_density.hip and asmc_moments.hip needs: the
// row-tile mixture evaluation, small host helpers of the launchers, the path switches, and what asmc_pcn.hip defines for the
// drivers: the padding helpers, the kernels' modes and launch functions, the mutation read-back.
#pragma once
#include <stdlib.h>

#include "asmc_common.h"
#include "asmc_tile.h"
#include "asmc_pcn_dev.h"

// =============================================================================================
// LDS row tiles
// =============================================================================================
// diagonal-mixture log-density of the row stored (as T) at `row`
template <typename T>
__device__ __forceinline__ double mixture_eval(const MixDev& m, int d, const char* row) {
    double best = -INFINITY;
    double terms[ASMC_MAX_COMPONENTS];
    const int C = m.C;
    for (int c = 0; c < C; c++) {
        double q = 0.0;
        const double* mu = m.mu + (size_t)c * d;
        const double* pr = m.prec + (size_t)c * d;
        for (int j = 0; j < d; j++) {
            const double t = row_get<T>(row, j) - mu[j];
            q = fma(t * t, pr[j], q);
        }
        const double v = m.logw[c] - 0.5 * q;
        terms[c] = v;
        best = fmax(best, v);
    }
    if (C == 1) return terms[0];
    if (best == -INFINITY) {  // every term -inf or NaN (fmax skips a NaN): their sum - -inf, or NaN for a row with a NaN coordinate
        double t = 0.0;
        for (int c = 0; c < C; c++) t += terms[c];
        return t;
    }
    double s = 0.0;
    for (int c = 0; c < C; c++) s += exp(terms[c] - best);
    return best + log(s);
}

__device__ __forceinline__ void wave_lds_sync() {
    // each wave owns its LDS tile: ordering within the wave is enough (no s_barrier, waves run decoupled)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

static int pick_vec(int rowbytes, const void* p0, const void* p1) {
    const uintptr_t a = (uintptr_t)p0 | (uintptr_t)p1;
    if (rowbytes % 16 == 0 && a % 16 == 0) return 16;
    if (rowbytes % 8 == 0 && a % 8 == 0) return 8;
    return 4;
}

static int waves_for_lds(size_t per_wave_bytes, size_t* lds_bytes_out) {
    const size_t budget = 160 * 1024 - 1024 - BM_TAB_N * 16;  // (the block's Box-Muller tables sit next to the tiles)
    int w = ASMC_BLOCK / 64;
    while (w > 1 && per_wave_bytes * (size_t)w > budget) w >>= 1;
    *lds_bytes_out = per_wave_bytes * (size_t)w;
    return w;
}

static int check_mixture(const asmc_mixture& m) {
    ASMC_REQUIRE(m.n_components >= 1 && m.n_components <= ASMC_MAX_COMPONENTS, "mixture: bad component count");
    ASMC_REQUIRE(m.logw_dev && m.mu_dev && m.prec_dev, "mixture: null device pointer");
    return ASMC_OK;
}

// next width with kernels of its own (register-resident: 4 .. 32, matrix-core: 64 / 128); 0: none
static int pcn_pad_dim(int d) {
    const int widths[] = {4, 8, 16, 32, 64, 128};
    for (int D : widths)
        if (d <= D) return D;
    return 0;
}

// The path switches of the pCN family.  Read on every call: the tests flip them inside one process.
static inline bool pcn_env_generic() { return getenv("ASMC_PCN_GENERIC") != nullptr; }  // no register-resident / matrix-core kernels
static inline bool pcn_env_nopad() { return getenv("ASMC_PCN_NOPAD") != nullptr; }      // no zero-padding to the next width
static inline bool pcn_env_xstate() { return getenv("ASMC_PCN_XSTATE") != nullptr; }    // no whitened-state stepping
static inline bool pcn_env_aos() { return getenv("ASMC_PCN_AOS") != nullptr; }          // no coordinate-major scratch

// ---- zero-padding to the next supported width (asmc_pcn.hip: the scheme, its kernels) ----
// grows ctx->d_xpad to `need` bytes (synchronises `st` first); `what`: the error text when the device has no room for it
int pcn_xpad_reserve(asmc_ctx* ctx, size_t need, hipStream_t st, const char* what);
// rows of d elements <-> rows of D >= d elements (zeros beyond d), n rows of x_dtype
int launch_pad_rows(asmc_ctx* ctx, int64_t n, int d, int D, int x_dtype, const void* src, void* dst, hipStream_t st);
int launch_unpad_rows(asmc_ctx* ctx, int64_t n, int d, int D, int x_dtype, const void* src, void* dst, hipStream_t st);
// The padded problem in ctx->d_xpad: the tables of `src` (a d-dimensional reference and its densities) padded to D at the
// head, the zero-padded copy of the rows x behind them.  n_mix: how many density tables the caller uses - 3 (ll, lp, lq),
// 2 (ll, lp: the proposal density is a flow) or 0 (the proposal half of the split path, which also gets a second row buffer
// xq for x' before the padding is stripped).
struct PcnPadded {
    double *mu, *L, *Linv;  // [D], [D, D], [D, D]
    double* mix;            // 3 x (mu[C_max, D] | prec[C_max, D])
    void *xp, *xq;
};
int pcn_pad_problem(asmc_ctx* ctx, int64_t n, int d, int D, int x_dtype, const void* x, const PcnDev& src, int n_mix, hipStream_t st,
                    PcnPadded* out);
// the same from a call's parameters: *p2 = *prm at dimension D, pointing at the padded tables; *xp: the padded rows
int pcn_pad_params(asmc_ctx* ctx, int64_t n, const void* x, const asmc_pcn_params* prm, int D, int n_mix, hipStream_t st,
                   asmc_pcn_params* p2, void** xp);

// ---- the step kernels' launch interface (asmc_pcn.hip), as the drivers of asmc_pcn_drive.hip see it ----
// The register-resident and the generic kernels are templates over the storage type; these functions turn the call's x_dtype into
// that argument, once.
//
// Modes of k_pcn_reg (pd.mode):
// MODE 0: one pCN step on x (whiten, propose, un-whiten, evaluate, accept)            — any built-in target
// MODE 1: one pCN step on the WHITENED state y = Linv (x - mu) carried in the x buffer: y' = a y + rho xi needs
//         no mat-vec, x' = mu + L y' is formed four rows at a time and consumed on the fly by the three
//         (single-component) quadratic forms, so it is never materialised: one mat-vec per step instead of two
// MODE 2: x -> y in place (start of a mutation);  MODE 3: y -> x in place + re-evaluate ll/lp/lq at the stored x
#define PCN_X_STEP 0
#define PCN_Y_STEP 1
#define PCN_WHITEN 2
#define PCN_UNWHITEN 3
#define PCN_UNWHITEN_X 4  // y -> x in place, carried ll/lp/lq untouched (flow-proposal path)
#define PCN_X_STEP_T 5    // PCN_X_STEP / PCN_Y_STEP with the Student-t reference (tpCN), selected at compile time
#define PCN_Y_STEP_T 6
// whitened state kept COORDINATE-MAJOR in a scratch buffer (ys[j * n_pad + i]) for the length of a mutation: the step
// kernel then needs no LDS staging at all (lane i reads 8 B of 64 consecutive particles per coordinate: 512-B coalesced
// loads straight into registers), so its occupancy is set by registers (3 waves/SIMD) instead of the 17 KB LDS tile
// (2 waves/SIMD), and rejected proposals cost no store.  x itself is only read by the first and written by the last.
#define PCN_WHITEN_S 7      // x (row-major) -> ys
#define PCN_Y_STEP_S 8      // step on ys
#define PCN_Y_STEP_TS 9     // ... Student-t reference
#define PCN_UNWHITEN_S 10   // ys -> x (row-major), ll / lp / lq re-evaluated at the stored x
#define PCN_UNWHITEN_XS 11  // ys -> x (row-major), carried ll / lp / lq untouched (flow-proposal path)
// proposal half of the split path (arbitrary Python callables evaluate the densities between propose and accept):
// x' -> the row-major buffer in p.ys, twice the reference's correction at y and y' -> the ll / lp arguments
#define PCN_X_PROPOSE 12
#define PCN_X_PROPOSE_T 13
// the same for 16 < d < 32 on the D = 32 kernel: rows of d elements, coordinates d..31 held at zero, tables padded with
// the identity (the generic LDS kernel needs 0.5-1.1 ms per proposal there, this one 0.3 ms)
#define PCN_X_PROPOSE_PAD 14
#define PCN_X_PROPOSE_PAD_T 15
// coordinate-major whitened-state step for densities with several mixture components: x' = mu + L y' is materialised in
// a second register array and handed to the general mixture evaluation (PCN_Y_STEP_S folds it into three quadratic
// forms on the fly, which only works for single Gaussians); still one mat-vec per step and no LDS
#define PCN_Y_STEP_SG 16
#define PCN_Y_STEP_TSG 17
// Modes of k_pcn_reg_flow - flow-proposal pCN on the whitened state, split around the flow's log-density kernel (asmc_flow.hip):
//   PCN_FLOW_PROPOSE  y' = a y + rho xi;  x' = mu + L y'  -> x_prop tile, ll'(x'), lp'(x') (built-in targets)
//   PCN_FLOW_ACCEPT   regenerates y' from the same Philox counters (no y' round trip through HBM), reads
//                     ll', lp', lq' and accepts: y <- y' (accepted rows only), carried log-probs updated
#define PCN_FLOW_PROPOSE 0
#define PCN_FLOW_ACCEPT 1
#define PCN_FLOW_PROPOSE_S 2  // the same with y coordinate-major in p.ys (see PCN_*_S above): propose stages only x'
#define PCN_FLOW_ACCEPT_S 3   // through LDS, accept touches no LDS at all
#define PCN_FLOW_PROPOSE_SX 4 // PCN_FLOW_PROPOSE_S without the built-in densities: the proposal half of the whitened-state
                              // split session, whose densities come from the caller (arbitrary Python callables)
#define PCN_FLOW_ACCEPT_SJ 5  // PCN_FLOW_ACCEPT_S with a carried log-Jacobian (chain in a preconditioned space): the two
                              // arrays arrive through the y / x_prop parameters, which coordinate-major accept does not use
// PCN_FLOW_PROPOSE_SX whose proposal lives in a preconditioned space z = T(x) (reference
// transforms.py:294-316 inside smc/minipcn.py:105-119): the inverse transform x' = T^-1(z') and its log-Jacobian are
// applied to the register-resident proposal, and - when the proposal flow's data transform shares T's bounded stage -
// log q(x') is evaluated from z' in the same pass (asmc_mixture_logpdf_premap's arithmetic).  x' goes to x_prop, log|J| to
// ll_new, log q to lp_new; lq_new carries the packed table (TRTAB_* in asmc_pcn.hip).  One variant per bounded stage.
#define PCN_FLOW_PROPOSE_SXT_LOGIT 6
#define PCN_FLOW_PROPOSE_SXT_PROBIT 7
// k_pcn_reg<T, D, NOISE, pd.mode> where the width has one, the generic fused step (k_pcn_step<T, VEC, 0>) otherwise
int pcn_step_launch(asmc_ctx* ctx, int64_t n, int x_dtype, void* x, double* ll, double* lp, double* lq, const PcnDev& pd,
                    const double* rho_ptr, uint32_t step, long long* block_counts, int* grid_out, hipStream_t st);
// the generic kernel's proposal half (k_pcn_step<T, VEC, 1>): x' -> x_prop, the reference's corrections -> qf_old, qf_new
int pcn_generic_propose_launch(asmc_ctx* ctx, int64_t n, int x_dtype, const void* x, void* x_prop, double* qf_old, double* qf_new,
                               const PcnDev& pd, const double* rho_ptr, uint32_t step, int* grid_out, hipStream_t st);
// k_pcn_reg_flow<T, pd.d, pd.noise, mode>, mode one of PCN_FLOW_*
int pcn_reg_flow_launch(asmc_ctx* ctx, int64_t n, int x_dtype, int mode, void* y, void* x_prop, double* ll, double* lp, double* lq,
                        double* ll_new, double* lp_new, const double* lq_new, const PcnDev& pd, const double* rho_ptr, uint32_t step,
                        long long* block_counts, int* grid_out, hipStream_t st);
int pcn_set_scalar_launch(asmc_ctx* ctx, double* cell, double v, hipStream_t st);
// the split path's accept decision: clears the count cell ctx->d_keys[0], then flags -> ctx->d_flags, carried scalars updated
int pcn_accept_flags_launch(asmc_ctx* ctx, int64_t n, double* ll, double* lp, double* lq, const double* ll_new, const double* lp_new,
                            const double* lq_new, double* lj_old, const double* lj_new, const double* qf_old, const double* qf_new,
                            double beta, uint64_t seed, uint64_t gid0, uint32_t step, hipStream_t st);
int launch_copy_flagged(asmc_ctx* ctx, int64_t n, int d, int x_dtype, void* x, const void* x_prop, const unsigned char* flags,
                        hipStream_t st);
// k_pcn_adapt behind the exchange of the last fused step of a sharded call (nobody's prologue follows it): the exchanged cells,
// the step size the step used (rho_hist[t])
int pcn_adapt_exchanged_launch(asmc_ctx* ctx, int t, double target, int adapt, int lag, hipStream_t st);
// the transform epilogue's table (TRTAB_*) -> d_tab, from the device-resident transform / premap / mixture tables
int pcn_trtab_pack_launch(asmc_ctx* ctx, int d, const asmc_transform* t, const double* premap_dev, const asmc_mixture* qmix,
                          int minus_logj, double* d_tab, hipStream_t st);
// gathers the caller's tables into ctx->d_ptab (rho_cell != NULL: the call's starting step size rides along)
int pack_pcn_tables(asmc_ctx* ctx, const PcnDev& pd, hipStream_t st, double* rho_cell = nullptr, double rho = 0.0);
// points pd.gam at step `step`'s scale variates (tpCN), drawing the next batch when they are not there
int pcn_prepare_gamma(asmc_ctx* ctx, int64_t n, PcnDev& pd, uint32_t step, hipStream_t st);
// closes step t: accept count (exchanged through the hook when one is installed), history, adaptation
int pcn_close_step(asmc_ctx* ctx, hipStream_t st, int grid, const long long* d_block, int64_t n, int t, long long* d_counts,
                   double* d_rho, double* d_rho_hist, double target, int adapt, int last = 1);
bool pcn_reg_supported(int d, size_t elem, const void* x);
int pcn_generic_check(int d, int x_dtype);
// coordinate-major scratch for the whitened state of one mutation; false: no room (callers stay on the row-major path)
bool pcn_ensure_ysoa(asmc_ctx* ctx, int64_t n, int d, int x_dtype, PcnDev& pd, hipStream_t st, bool with_scratch = false);
// a mutation call's read-back into the pinned HP_PCN_* cells, the NaN count of the carried log q beside it, and the hand-out
int pcn_enqueue_lq_check(asmc_ctx* ctx, int64_t n, const double* lq, hipStream_t st);
int pcn_readback_enqueue(asmc_ctx* ctx, int n_steps, const void* d_bad, hipStream_t st);
void pcn_readback_handout(asmc_ctx* ctx, int n_steps, bool flow, bool lq_checked, double* rho_out_host, int64_t* n_accept_host,
                          double* rho_hist_host);
