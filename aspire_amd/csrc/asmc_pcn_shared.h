// asmc_pcn_shared.h — what more than one of asmc_pcn.hip, asmc_density.hip and asmc_moments.hip needs: the row-tile mixture
// evaluation, small host helpers of the launchers, the path switches and the padding helpers (defined in asmc_pcn.hip).
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
