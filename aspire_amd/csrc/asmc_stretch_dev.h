// asmc_stretch_dev.h — what the ensemble moves share (asmc_stretch.hip: the stretch move; asmc_ensemble.hip: the DE and snooker
// moves): the counter-keyed split, the slot-to-walker map, the per-slot draw blocks and the accept step.  One copy: the split of
// nsplits = 2 and the accept of asmc_stretch_* are the S = 2, tag 0x60000000 instance of the code below, bit for bit.
// Specification: include/asmc.h (asmc_stretch_*, asmc_ensemble_*).
#pragma once
#include "asmc_pcn_dev.h"

#define STRETCH_TAG_DRAW 0x60000000u   // counter word 3 of the stretch move's per-slot draws (| shard)
#define ENSEMBLE_TAG_DRAW 0x70000000u  // ... of the DE and snooker moves' (| shard)
#define STRETCH_TAG_SPLIT 0xA0000000u  // counter word 3 of the split's Feistel round function (| shard)
#define STRETCH_ROUNDS 4
#define STRETCH_MAX_SHARD 0x10000000u

struct StretchArgs {
    int64_t n;        // walkers of the ensemble (this rank's shard)
    int64_t n_half;   // slots of the active group: ceil((n - h) / S)
    int64_t n_other;  // S = 2: walkers of the other half, (n + h) / 2
    uint32_t half;    // h: the active group
    uint32_t lg_s;    // log2 S: 1 (halves) or 2 (four groups)
    uint32_t lg_b;    // counter word 2 of draw block b is (b << lg_b) | h: 1 (stretch move), 2 (DE and snooker moves)
    uint32_t tag;     // counter word 3 of the per-slot draws, shard included
    uint32_t hbits;   // Feistel half width: ceil(ceil(log2 n) / 2)
    uint32_t step;    // counter word 1 of every draw of this step
    uint32_t shard;   // low bits of counter word 3 (this rank: each shard is its own ensemble)
    uint32_t k0, k1;  // Philox key: the mutation's seed
    double a;         // stretch scale; DE: g0; snooker: gammas
    double b;         // DE: sigma
    int d, lg_tpr;    // row width; log2 of the lanes that share one row in the row passes
};

// ---- the split: Feistel network on 2 hbits bits, round function = word 0 of one Philox block ------------------------------
__device__ __forceinline__ uint32_t stretch_round(const StretchArgs& s, uint32_t r, uint32_t v) {
    uint32_t w[4];
    philox4x32_10(v, s.step, r, STRETCH_TAG_SPLIT | s.shard, s.k0, s.k1, w);
    return w[0] & ((1u << s.hbits) - 1u);
}

// sigma^-1: the inverse network, walked until the value falls inside [0, n) (cycle walking keeps it a bijection of [0, n))
__device__ __forceinline__ uint32_t stretch_sigma_inv(const StretchArgs& s, uint32_t v) {
    const uint32_t mask = (1u << s.hbits) - 1u;
    do {
        uint32_t L = v >> s.hbits, R = v & mask;
#pragma unroll
        for (int r = STRETCH_ROUNDS - 1; r >= 0; r--) {
            const uint32_t R0 = L;
            L = R ^ stretch_round(s, (uint32_t)r, L);
            R = R0;
        }
        v = (L << s.hbits) | R;
    } while ((int64_t)v >= s.n);
    return v;
}

// block b of the per-slot draws of slot m (what each block holds: asmc_stretch.hip, asmc_ensemble.hip); block 0, words 2 and 3,
// is the accept variate of every move
__device__ __forceinline__ void stretch_block(const StretchArgs& s, uint64_t m, uint32_t b, uint32_t w[4]) {
    philox4x32_10((uint32_t)m, s.step, (b << s.lg_b) | s.half, s.tag, s.k0, s.k1, w);
}

// slot m of group g: the walker sigma^-1(S m + g)
__device__ __forceinline__ uint32_t stretch_member(const StretchArgs& s, uint64_t m, uint32_t g) {
    return stretch_sigma_inv(s, (uint32_t)((m << s.lg_s) + g));
}
__device__ __forceinline__ uint32_t stretch_walker(const StretchArgs& s, uint64_t m) { return stretch_member(s, m, s.half); }

// floor(((w0 << 32) | w1) K / 2^64) for K < 2^32, exact
__device__ __forceinline__ uint64_t stretch_index(uint32_t w0, uint32_t w1, uint64_t K) {
    const uint64_t hi = (uint64_t)w0 * K;
    const uint64_t lo = (uint64_t)w1 * K;
    return (hi + (lo >> 32)) >> 32;
}

// the accept step of one block of slots: tempered log-target of y and of x_k, accept, copy y[m] into row k and the new densities
// into the carried arrays; the accepts go to the step's device-resident counter
template <typename T>
__device__ __forceinline__ void stretch_accept_body(T* __restrict__ x, const StretchArgs& s, const T* __restrict__ y,
                                                    const double* __restrict__ logf, double beta, double* __restrict__ ll,
                                                    double* __restrict__ lp, double* __restrict__ lq, double* __restrict__ lj,
                                                    const double* __restrict__ ll_new, const double* __restrict__ lp_new,
                                                    const double* __restrict__ lq_new, const double* __restrict__ lj_new,
                                                    unsigned long long* __restrict__ count) {
    __shared__ int64_t s_k[ASMC_BLOCK];  // the walker an accepted slot moves, -1: rejected
    const int64_t m0 = (int64_t)blockIdx.x * ASMC_BLOCK;
    const int64_t m = m0 + threadIdx.x;
    bool acc = false;
    if (m < s.n_half) {
        const int64_t k = stretch_walker(s, (uint64_t)m);
        uint32_t w[4];
        stretch_block(s, (uint64_t)m, 0, w);
        const double u = u01_from_words(w[2], w[3]);
        double nlp = log_p_t(ll_new[m], lp_new[m], lq_new[m], beta);
        double olp = log_p_t(ll[k], lp[k], lq[k], beta);
        if (lj != nullptr) {  // a chain in a preconditioned space: log|det dT^-1/dz| joins the log-target, NaN / +inf -> -inf again
            nlp = log_p_t_guard(nlp + lj_new[m]);
            olp = log_p_t_guard(olp + lj[k]);
        }
        const double lnpdiff = logf[m] + nlp - olp;  // emcee's order: (f + new) - old
        acc = lnpdiff > log(u);
        if (acc) {
            ll[k] = ll_new[m];
            lp[k] = lp_new[m];
            lq[k] = lq_new[m];
            if (lj != nullptr) lj[k] = lj_new[m];
        }
        s_k[threadIdx.x] = acc ? k : -1;
    }
    const unsigned long long ballot = __ballot(acc);
    if ((threadIdx.x & (ASMC_WAVE - 1)) == 0 && ballot != 0ull) atomicAdd(count, (unsigned long long)__popcll(ballot));
    __syncthreads();
    const int64_t rows = s.n_half - m0 < ASMC_BLOCK ? s.n_half - m0 : ASMC_BLOCK;
    const int tpr = 1 << s.lg_tpr;
    for (int64_t r = threadIdx.x >> s.lg_tpr; r < rows; r += ASMC_BLOCK >> s.lg_tpr) {
        const int64_t k = s_k[r];
        if (k < 0) continue;
        const T* __restrict__ yr = y + (m0 + r) * s.d;
        T* __restrict__ xr = x + k * s.d;
        for (int c = threadIdx.x & (tpr - 1); c < s.d; c += tpr) xr[c] = yr[c];
    }
}

// the arguments every entry point shares; S = 2 or 4 groups, `tag` without the shard
static inline int stretch_args(asmc_ctx* ctx, int64_t n, int64_t n_min, int d, int x_dtype, int nsplits, int group, uint32_t tag,
                               uint64_t seed, uint32_t shard, uint32_t step, int t, StretchArgs& s) {
    ASMC_REQUIRE(ctx != nullptr, "null ctx");
    ASMC_REQUIRE(n >= n_min && n < (1LL << 31) && d > 0 && d <= ASMC_MAX_DIMS,
                 n_min == 2 ? "bad sizes (2 <= n < 2^31, 0 < d <= ASMC_MAX_DIMS)" : "bad sizes (4 <= n < 2^31, 0 < d <= ASMC_MAX_DIMS)");
    ASMC_REQUIRE(x_dtype == ASMC_F64 || x_dtype == ASMC_F32, "bad x_dtype");
    ASMC_REQUIRE(nsplits == 2 || nsplits == 4, "nsplits must be 2 or 4");
    ASMC_REQUIRE(group >= 0 && group < nsplits, nsplits == 2 ? "half must be 0 or 1" : "group must be 0 .. nsplits - 1");
    ASMC_REQUIRE(shard < STRETCH_MAX_SHARD, "shard must be < 2^28");
    ASMC_REQUIRE(t >= 0 && t < ASMC_MAX_PCN_STEPS, "step index t out of range");
    memset(&s, 0, sizeof(s));
    s.n = n;
    s.half = (uint32_t)group;
    s.lg_s = nsplits == 2 ? 1u : 2u;
    s.lg_b = tag == STRETCH_TAG_DRAW ? 1u : 2u;
    s.tag = tag | shard;
    s.n_half = (n - group + nsplits - 1) / nsplits;
    s.n_other = (n + group) / 2;
    uint32_t bits = 0;
    while ((1LL << bits) < n) bits++;
    s.hbits = (bits + 1) / 2;
    s.step = step;
    s.shard = shard;
    s.k0 = (uint32_t)seed;
    s.k1 = (uint32_t)(seed >> 32);
    s.d = d;
    s.lg_tpr = 0;
    while ((1 << s.lg_tpr) < d && s.lg_tpr < 6) s.lg_tpr++;
    return ASMC_OK;
}
