// asmc_chain.hip - the chain recorder of the "minipcn" / "emcee" MCMC samplers (include/asmc.h, ABI 28).
//
// An MCMC run keeps every step of every walker in a device chain [n_slots, n, pitch].  A slot is written once, from
//   - row-major rows (the generic pCN path, the stretch move, asmc_pcn_mutate where it steps on x): the copy kernel below, or
//     asmc_transform_inverse's kernels with the slot as their output when the chain runs in z = T(x);
//   - the whitened coordinate-major state of a session: the un-whitening launch of asmc_pcn_ysplit_end (asmc_pcn_drive.hip) with the
//     slot as its output, so that a recorded row is what ending the session at that step returns.
// The copy is memory bound (n d s bytes in, n d s out): one 16-byte vector per lane and consecutive lanes on consecutive
// vectors where the row length, the pitch and both pointers are multiples of 16 bytes; element-wise, equally coalesced,
// otherwise.  Every index is 64-bit; elements between d and the pitch, and rows beyond n, are never touched.  No atomics.
#include "asmc_common.h"

#define CHAIN_GRID_CAP 8192  // blocks of the grid-stride copy (256 CUs x 8 resident blocks x 4 rounds)

// `units` per row of the source (16-byte vectors or elements), `pitch_units` per row of the slot
template <typename V>
__global__ __launch_bounds__(ASMC_BLOCK) void k_chain_rows(int64_t n, int64_t units, int64_t pitch_units, const V* __restrict__ src,
                                                           V* __restrict__ dst, const double* __restrict__ ll,
                                                           const double* __restrict__ lp, double* __restrict__ ll_out,
                                                           double* __restrict__ lp_out) {
    const int64_t stride = (int64_t)gridDim.x * ASMC_BLOCK;
    const int64_t i0 = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x;
    const int64_t total = n * units;
    if (pitch_units == units) {
        for (int64_t e = i0; e < total; e += stride) dst[e] = src[e];
    } else {
        for (int64_t e = i0; e < total; e += stride) {
            const int64_t r = e / units;
            dst[r * pitch_units + (e - r * units)] = src[e];
        }
    }
    if (ll_out != nullptr)
        for (int64_t i = i0; i < n; i += stride) ll_out[i] = ll[i];
    if (lp_out != nullptr)
        for (int64_t i = i0; i < n; i += stride) lp_out[i] = lp[i];
}

static int chain_check(const asmc_ctx* ctx, const asmc_chain_target* c) {
    ASMC_REQUIRE(ctx != nullptr && c != nullptr, "null pointer");
    ASMC_REQUIRE(c->x_dev != nullptr, "chain: null x_dev");
    ASMC_REQUIRE(c->x_dtype == ASMC_F64 || c->x_dtype == ASMC_F32, "chain: bad x_dtype");
    ASMC_REQUIRE(c->n > 0 && c->d > 0 && c->d <= ASMC_MAX_DIMS && c->n_slots > 0, "chain: bad sizes");
    ASMC_REQUIRE(c->pitch >= c->d, "chain: the pitch is shorter than a row");
    return ASMC_OK;
}

static inline size_t chain_elem(const asmc_chain_target* c) { return c->x_dtype == ASMC_F64 ? 8 : 4; }
static inline char* chain_slot(const asmc_chain_target* c, int64_t slot) {
    return static_cast<char*>(c->x_dev) + (size_t)slot * (size_t)c->n * (size_t)c->pitch * chain_elem(c);
}

int asmc_chain_rows_launch(asmc_ctx* ctx, const asmc_chain_target* c, int64_t slot, const void* src, const double* ll,
                           const double* lp, hipStream_t st) {
    ASMC_REQUIRE(src != nullptr, "null source rows");
    ASMC_REQUIRE((c->ll_dev == nullptr || ll != nullptr) && (c->lp_dev == nullptr || lp != nullptr), "null source densities");
    const size_t elem = chain_elem(c);
    char* dst = chain_slot(c, slot);
    double* ll_out = c->ll_dev ? c->ll_dev + (size_t)slot * (size_t)c->n : nullptr;
    double* lp_out = c->lp_dev ? c->lp_dev + (size_t)slot * (size_t)c->n : nullptr;
    const size_t rowb = (size_t)c->d * elem, pitchb = (size_t)c->pitch * elem;
    const bool vec = rowb % 16 == 0 && pitchb % 16 == 0 && ((uintptr_t)src | (uintptr_t)dst) % 16 == 0;
    const int64_t units = vec ? (int64_t)(rowb / 16) : c->d;
    const int64_t pitch_units = vec ? (int64_t)(pitchb / 16) : c->pitch;
    const int grid = grid_for(c->n * units, ASMC_BLOCK, CHAIN_GRID_CAP);
    if (vec)
        ASMC_LAUNCH(ctx, st, "k_chain_rows", k_chain_rows<uint4>, dim3(grid), dim3(ASMC_BLOCK), 0, st, c->n, units, pitch_units,
                    (const uint4*)src, (uint4*)dst, ll, lp, ll_out, lp_out);
    else if (elem == 8)
        ASMC_LAUNCH(ctx, st, "k_chain_rows", k_chain_rows<double>, dim3(grid), dim3(ASMC_BLOCK), 0, st, c->n, units, pitch_units,
                    (const double*)src, (double*)dst, ll, lp, ll_out, lp_out);
    else
        ASMC_LAUNCH(ctx, st, "k_chain_rows", k_chain_rows<float>, dim3(grid), dim3(ASMC_BLOCK), 0, st, c->n, units, pitch_units,
                    (const float*)src, (float*)dst, ll, lp, ll_out, lp_out);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

// the carried densities alone (sources whose rows another kernel writes)
int asmc_chain_scalars_launch(asmc_ctx* ctx, const asmc_chain_target* c, int64_t slot, const double* ll, const double* lp,
                                hipStream_t st) {
    if (c->ll_dev == nullptr && c->lp_dev == nullptr) return ASMC_OK;
    ASMC_REQUIRE((c->ll_dev == nullptr || ll != nullptr) && (c->lp_dev == nullptr || lp != nullptr), "null source densities");
    double* ll_out = c->ll_dev ? c->ll_dev + (size_t)slot * (size_t)c->n : nullptr;
    double* lp_out = c->lp_dev ? c->lp_dev + (size_t)slot * (size_t)c->n : nullptr;
    const int grid = grid_for(c->n, ASMC_BLOCK, CHAIN_GRID_CAP);
    ASMC_LAUNCH(ctx, st, "k_chain_rows", k_chain_rows<double>, dim3(grid), dim3(ASMC_BLOCK), 0, st, c->n, (int64_t)0, (int64_t)0,
                (const double*)nullptr, (double*)nullptr, ll, lp, ll_out, lp_out);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

extern "C" {

int asmc_chain_record(asmc_ctx* ctx, const asmc_chain_target* c, int64_t slot, int source, const void* src, const double* ll,
                      const double* lp, const asmc_pcn_params* prm, const asmc_transform* t, asmc_stream stream) {
    int rc = chain_check(ctx, c);
    if (rc) return rc;
    ASMC_REQUIRE(slot >= 0 && slot < c->n_slots, "slot outside the chain");
    ASMC_REQUIRE(source == ASMC_CHAIN_ROWS || source == ASMC_CHAIN_YS, "bad source");
    hipStream_t st = as_stream(stream);
    if (source == ASMC_CHAIN_ROWS && t == nullptr) return asmc_chain_rows_launch(ctx, c, slot, src, ll, lp, st);
    ASMC_REQUIRE(c->pitch == c->d, "this source writes whole rows back to back: pitch == d");
    if (source == ASMC_CHAIN_ROWS) {
        ASMC_REQUIRE(src != nullptr && t->d == c->d, "null source rows / transform of another d");
        rc = asmc_transform_inverse(ctx, c->n, c->x_dtype, src, chain_slot(c, slot), nullptr, t, stream);
    } else {
        ASMC_REQUIRE(prm != nullptr && t == nullptr, "the session's parameters, no transform");
        ASMC_REQUIRE(prm->d == c->d && prm->x_dtype == c->x_dtype, "the session's d / dtype differ from the chain's");
        rc = asmc_pcn_ysplit_unwhiten(ctx, c->n, chain_slot(c, slot), prm, false, st);
    }
    if (rc) return rc;
    return asmc_chain_scalars_launch(ctx, c, slot, ll, lp, st);
}

int asmc_chain_set(asmc_ctx* ctx, const asmc_chain_target* c) {
    int rc = chain_check(ctx, c);
    if (rc) return rc;
    ASMC_REQUIRE(c->ll_dev != nullptr && c->lp_dev != nullptr, "a step loop's target records the densities too");
    ASMC_REQUIRE(c->stride >= 1 && c->slot0 >= 0 && c->slot0 < c->n_slots, "bad stride / first slot");
    // a width the loop zero-pads (asmc_pcn.hip: the next of 4, 8, 16, 32, 64, 128) un-whitens into scratch rows of that width
    int D = 0;
    for (int w : {4, 8, 16, 32, 64, 128})
        if (D == 0 && c->d <= w) D = w;
    // at a width with whitened-state kernels of its own the un-whitening launch writes the slot itself: whole rows back to back at
    // 16-byte boundaries (such a row is a multiple of 16 bytes, so every slot starts on one when the chain does); every other width
    // reaches the slot through the copy / un-padding kernels, which take any address
    ASMC_REQUIRE(c->pitch == c->d, "a step loop's target: pitch == d");
    ASMC_REQUIRE(D != c->d || (uintptr_t)c->x_dev % 16 == 0, "a step loop's target at d = 4, 8, 16, 32, 64, 128: a 16-byte aligned chain");
    const size_t rows = D > c->d ? (size_t)c->n * (size_t)D * chain_elem(c) : 0;
    if (rows > ctx->chain_rows_bytes) {
        ASMC_HIP(hipDeviceSynchronize());
        if (ctx->d_chain_rows) (void)hipFree(ctx->d_chain_rows);
        ctx->d_chain_rows = nullptr;
        ctx->chain_rows_bytes = 0;
        if (hipMalloc(&ctx->d_chain_rows, rows) != hipSuccess) {
            (void)hipGetLastError();
            asmc_set_error("asmc_chain_set: no device memory for %zu bytes of padded rows", rows);
            return ASMC_ERR_NOMEM;
        }
        ctx->chain_rows_bytes = rows;
    }
    if (c->n > ctx->chain_lq_n) {
        ASMC_HIP(hipDeviceSynchronize());
        if (ctx->d_chain_lq) (void)hipFree(ctx->d_chain_lq);
        ctx->d_chain_lq = nullptr;
        ctx->chain_lq_n = 0;
        if (hipMalloc(&ctx->d_chain_lq, sizeof(double) * (size_t)c->n) != hipSuccess) {
            (void)hipGetLastError();
            asmc_set_error("asmc_chain_set: no device memory for %lld doubles of scratch", (long long)c->n);
            return ASMC_ERR_NOMEM;
        }
        ctx->chain_lq_n = c->n;
    }
    ctx->chain = *c;
    ctx->chain_on = 1;
    return ASMC_OK;
}

int asmc_chain_clear(asmc_ctx* ctx) {
    ASMC_REQUIRE(ctx != nullptr, "null ctx");
    ctx->chain_on = 0;
    return ASMC_OK;
}

}  // extern "C"
