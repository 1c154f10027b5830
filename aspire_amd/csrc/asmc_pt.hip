// asmc_pt.hip - parallel tempering of the "pt_minipcn" sampler (include/asmc.h, ABI 29): the replica exchange
// between the rungs of a tempered ensemble, and the reductions over a recorded log-likelihood chain from which the host forms
// the thermodynamic-integration and stepping-stone evidence.
//
// Both are memory kernels.  The exchange reads two log-likelihoods per pair of walkers and moves 2 rows (read and written) per
// accepted pair; the reductions read every kept log-likelihood twice (once for its rung's sums, once for the per-sample
// trapezoid) and write a few hundred doubles.  Every index is 64-bit.
#include "asmc_pcn_dev.h"

#define PT_TAG 0x50000000u  // counter word 3 of the exchange's uniforms (| r): no other stream of the library uses it (asmc.h)

// ---- replica exchange --------------------------------------------------------------------------------------------------------
// One group of G = 2^lg <= 4 consecutive lanes (so a group lies in one wave) per (pair, walker); the group's lanes hold the row's
// units u0, u0 + G, ... (16-byte vectors or elements) and consecutive groups hold consecutive walkers, so the 64-byte pieces a
// wave touches in one instruction make up whole rows over the loop.  Every lane forms the decision itself from the pair's two
// log-likelihoods and the pair's Philox block.  The lanes of a group execute the loads of ll in one instruction and lane 0 stores
// the exchanged ll behind a branch on the loaded values, so no lane can see a pair's ll after its exchange.
// G: the decision (a Philox block and an fp64 log) costs the same per lane whatever the lane moves, and with one lane per
// 16-byte vector it bounds the kernel.  Measured on MI355X at 8 x 128k x 32 fp64 (4 pairs of rungs per round, mean acceptance
// 0.77): G = 64 -> 16 lanes per row 0.352 ms, G = 8 0.184, G = 4 0.103 (3.6 TB/s of the rows it moves), G = 2 0.113, G = 1 0.221.
#define PT_SWAP_LG 2
template <typename V>
__global__ __launch_bounds__(ASMC_BLOCK) void k_pt_swap(int n_pairs, int par, int64_t W, int64_t units, int lg, V* x, double* ll,
                                                        double* lp, double* c0, double* c1, const double* __restrict__ betas,
                                                        uint32_t k0, uint32_t k1, uint32_t round, unsigned long long* counts) {
    __shared__ unsigned int s_cnt[ASMC_PT_MAX_RUNGS / 2];
    if (threadIdx.x < ASMC_PT_MAX_RUNGS / 2) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t t = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x;
    const int64_t grp = t >> lg;
    const int64_t u0 = t & (((int64_t)1 << lg) - 1);
    if (grp < (int64_t)n_pairs * W) {
        const int64_t p = grp / W, w = grp - p * W;
        const int r = par + 2 * (int)p;
        const int64_t ra = (int64_t)r * W + w, rb = ra + W;
        const double la = ll[ra], lb = ll[rb];
        V* __restrict__ xa = x + ra * units;  // (two different rows)
        V* __restrict__ xb = x + rb * units;
        uint32_t wd[4];
        philox4x32_10((uint32_t)w, (uint32_t)((unsigned long long)w >> 32), round, PT_TAG | (uint32_t)r, k0, k1, wd);
        const double logu = bm_log_unit(u01_from_words(wd[0], wd[1]));
        const double rhs = (betas[r] - betas[r + 1]) * (lb - la);
        if (isfinite(la) && isfinite(lb) && logu < rhs) {
            for (int64_t u = u0; u < units; u += (int64_t)1 << lg) {
                const V va = xa[u], vb = xb[u];
                xa[u] = vb;
                xb[u] = va;
            }
            if (u0 == 0) {
                ll[ra] = lb;
                ll[rb] = la;
                const double pa = lp[ra], pb = lp[rb];
                lp[ra] = pb;
                lp[rb] = pa;
                if (c0 != nullptr) {
                    const double a = c0[ra], b = c0[rb];
                    c0[ra] = b;
                    c0[rb] = a;
                }
                if (c1 != nullptr) {
                    const double a = c1[ra], b = c1[rb];
                    c1[ra] = b;
                    c1[rb] = a;
                }
                atomicAdd(&s_cnt[p], 1u);
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < n_pairs && s_cnt[threadIdx.x] != 0u)
        atomicAdd(&counts[par + 2 * (int)threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

// ---- evidence reductions -----------------------------------------------------------------------------------------------------
#define PT_EV_ITEMS 4  // samples per thread and grid-stride round the grid is sized for

// (max, sum, sum of squares) of exp(a - max): an element is {a, 1, 1}; the empty set {-inf, 0, 0}.  A set whose maximum is
// infinite keeps its count here and becomes NaN when the result is written (numpy: exp(a - max(a)) with inf - inf).
struct PtLse {
    double m, s1, s2;
};
__device__ __forceinline__ bool pt_lse_empty(const PtLse& a) { return a.s1 == 0.0 && a.m == -INFINITY; }
__device__ __forceinline__ PtLse pt_lse_merge(const PtLse& a, const PtLse& b) {
    if (pt_lse_empty(a)) return b;
    if (pt_lse_empty(b)) return a;
    PtLse o;
    o.m = (a.m != a.m || b.m != b.m) ? (a.m + b.m) : fmax(a.m, b.m);
    const double wa = a.m == o.m ? 1.0 : exp(a.m - o.m), wb = b.m == o.m ? 1.0 : exp(b.m - o.m);
    o.s1 = a.s1 * wa + b.s1 * wb;
    o.s2 = a.s2 * (wa * wa) + b.s2 * (wb * wb);
    return o;
}
__device__ __forceinline__ void pt_lse_add(PtLse& s, double a) {
    if (a <= s.m) {
        const double e = a == s.m ? 1.0 : exp(a - s.m);
        s.s1 += e;
        s.s2 += e * e;
    } else {  // a new maximum, the first element, or a NaN on either side
        const PtLse el = {a, 1.0, 1.0};
        s = pt_lse_merge(s, el);
    }
}

// (count, mean, centred second moment): Welford's update and Chan's merge
struct PtMom {
    double k, mean, m2;
};
__device__ __forceinline__ PtMom pt_mom_merge(const PtMom& a, const PtMom& b) {
    if (a.k == 0.0) return b;
    if (b.k == 0.0) return a;
    PtMom o;
    o.k = a.k + b.k;
    const double delta = b.mean - a.mean;
    o.mean = a.mean + delta * (b.k / o.k);
    o.m2 = a.m2 + b.m2 + delta * delta * (a.k * (b.k / o.k));
    return o;
}

__device__ __forceinline__ double pt_shfl(double v, int o) { return __shfl_xor(v, o, 64); }

// the four doubles of a thread -> the block's, in thread 0; MOM: a PtMom in v[0..2], else {sum, PtLse} in v[0..3]
template <bool MOM>
__device__ __forceinline__ void pt_merge4(double (&v)[4], const double (&o)[4]) {
    if (MOM) {
        const PtMom a = {v[0], v[1], v[2]}, b = {o[0], o[1], o[2]};
        const PtMom c = pt_mom_merge(a, b);
        v[0] = c.k;
        v[1] = c.mean;
        v[2] = c.m2;
    } else {
        const PtLse a = {v[1], v[2], v[3]}, b = {o[1], o[2], o[3]};
        const PtLse c = pt_lse_merge(a, b);
        v[0] += o[0];
        v[1] = c.m;
        v[2] = c.s1;
        v[3] = c.s2;
    }
}
template <bool MOM>
__device__ __forceinline__ void pt_wave_merge(double (&v)[4]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        // the lower lane of a pair merges (own, partner), the upper one (partner, own): both hold the same bits afterwards
        const bool upper = (threadIdx.x & o) != 0;
        double own[4] = {v[0], v[1], v[2], v[3]};
        double oth[4] = {pt_shfl(v[0], o), pt_shfl(v[1], o), pt_shfl(v[2], o), pt_shfl(v[3], o)};
        if (upper) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const double tmp = own[j];
                own[j] = oth[j];
                oth[j] = tmp;
            }
        }
        pt_merge4<MOM>(own, oth);
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = own[j];
    }
}
template <bool MOM>
__device__ __forceinline__ void pt_block_merge(double (&v)[4], double (*s_w)[4]) {
    pt_wave_merge<MOM>(v);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0)
        for (int j = 0; j < 4; j++) s_w[wave][j] = v[j];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int q = 1; q < ASMC_BLOCK / ASMC_WAVE; q++) {
            const double o[4] = {s_w[q][0], s_w[q][1], s_w[q][2], s_w[q][3]};
            pt_merge4<MOM>(v, o);
        }
}

// blockIdx.y = r < T: rung r's {sum ll, (max, S1, S2) of a = s_r ll}; blockIdx.y = T: (n, mean, M2) of ti = sum_r c_r ll[r, .]
// partials [T + 1][gridDim.x][4]
__global__ __launch_bounds__(ASMC_BLOCK) void k_pt_evidence(int T, int64_t stride, int64_t offset, int64_t n,
                                                            const double* __restrict__ ll, const double* __restrict__ coef,
                                                            double* __restrict__ partials) {
    __shared__ double s_w[ASMC_BLOCK / ASMC_WAVE][4];
    __shared__ double s_c[ASMC_PT_MAX_RUNGS];
    const int y = blockIdx.y;
    const int64_t step = (int64_t)gridDim.x * ASMC_BLOCK;
    const int64_t i0 = (int64_t)blockIdx.x * ASMC_BLOCK + threadIdx.x;
    double v[4];
    if (y < T) {
        const double* row = ll + (int64_t)y * stride + offset;
        const double s = coef[T + y];
        double sum = 0.0;
        PtLse acc = {-INFINITY, 0.0, 0.0};
        for (int64_t i = i0; i < n; i += step) {
            const double l = row[i];
            sum += l;
            pt_lse_add(acc, s * l);
        }
        v[0] = sum;
        v[1] = acc.m;
        v[2] = acc.s1;
        v[3] = acc.s2;
        pt_block_merge<false>(v, s_w);
    } else {
        if ((int)threadIdx.x < T) s_c[threadIdx.x] = coef[threadIdx.x];
        __syncthreads();
        PtMom acc = {0.0, 0.0, 0.0};
        const double* base = ll + offset;
        for (int64_t i = i0; i < n; i += step) {
            double ti = 0.0;
            for (int r = 0; r < T; r++) ti += s_c[r] * base[(int64_t)r * stride + i];
            acc.k += 1.0;
            const double delta = ti - acc.mean;
            acc.mean += delta / acc.k;
            acc.m2 += delta * (ti - acc.mean);
        }
        v[0] = acc.k;
        v[1] = acc.mean;
        v[2] = acc.m2;
        v[3] = 0.0;
        pt_block_merge<true>(v, s_w);
    }
    if (threadIdx.x == 0) {
        double* o = partials + ((int64_t)y * gridDim.x + blockIdx.x) * 4;
        for (int j = 0; j < 4; j++) o[j] = v[j];
    }
}

// one wave per row of the result: merges the row's block partials in a fixed order
__global__ __launch_bounds__(ASMC_WAVE) void k_pt_evidence_final(int T, int n_part, const double* __restrict__ partials,
                                                                 double* __restrict__ out) {
    const int y = blockIdx.x;
    const double* p = partials + (int64_t)y * n_part * 4;
    double v[4];
    if (y < T) {
        v[0] = 0.0;
        v[1] = -INFINITY;
        v[2] = 0.0;
        v[3] = 0.0;
        for (int b = threadIdx.x; b < n_part; b += ASMC_WAVE) {
            const double o[4] = {p[4 * b], p[4 * b + 1], p[4 * b + 2], p[4 * b + 3]};
            pt_merge4<false>(v, o);
        }
        pt_wave_merge<false>(v);
        if (isinf(v[1])) v[2] = v[3] = NAN;  // numpy: exp(a - max(a)) at an infinite maximum
    } else {
        v[0] = v[1] = v[2] = v[3] = 0.0;
        for (int b = threadIdx.x; b < n_part; b += ASMC_WAVE) {
            const double o[4] = {p[4 * b], p[4 * b + 1], p[4 * b + 2], 0.0};
            pt_merge4<true>(v, o);
        }
        pt_wave_merge<true>(v);
        v[3] = 0.0;
    }
    if (threadIdx.x == 0)
        for (int j = 0; j < 4; j++) out[4 * y + j] = v[j];
}

extern "C" {

int asmc_pt_swap(asmc_ctx* ctx, int T, int64_t W, int d, int x_dtype, void* x, double* ll, double* lp, double* c0, double* c1,
                 const double* betas, uint64_t seed, uint32_t round, int64_t* counts, asmc_stream stream) {
    ASMC_REQUIRE(ctx != nullptr && x != nullptr && ll != nullptr && lp != nullptr && betas != nullptr, "null pointer");
    ASMC_REQUIRE(T >= 1 && T <= ASMC_PT_MAX_RUNGS, "n_temps outside 1 .. ASMC_PT_MAX_RUNGS");
    ASMC_REQUIRE(W > 0 && d > 0 && d <= ASMC_MAX_DIMS, "bad n_walkers / d");
    ASMC_REQUIRE(x_dtype == ASMC_F64 || x_dtype == ASMC_F32, "bad x_dtype");
    ASMC_REQUIRE(counts != nullptr || T == 1, "null counts");
    const int par = (int)(round & 1u);
    const int n_pairs = (T - par) / 2;
    if (n_pairs <= 0) return ASMC_OK;
    const size_t elem = x_dtype == ASMC_F64 ? 8 : 4;
    const size_t rowb = (size_t)d * elem;
    const bool vec = rowb % 16 == 0 && (uintptr_t)x % 16 == 0;
    const int64_t units = vec ? (int64_t)(rowb / 16) : d;
    int lg = 0;
    while (lg < PT_SWAP_LG && ((int64_t)1 << lg) < units) lg++;
    const int64_t threads = ((int64_t)n_pairs * W) << lg;
    const int64_t grid = (threads + ASMC_BLOCK - 1) / ASMC_BLOCK;
    ASMC_REQUIRE(grid <= 0x7FFFFFFFLL, "too many walkers for one launch");
    hipStream_t st = as_stream(stream);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
    if (vec)
        ASMC_LAUNCH(ctx, st, "k_pt_swap", k_pt_swap<uint4>, dim3((unsigned)grid), dim3(ASMC_BLOCK), 0, st, n_pairs, par, W, units, lg,
                    (uint4*)x, ll, lp, c0, c1, betas, k0, k1, round, cnt);
    else if (elem == 8)
        ASMC_LAUNCH(ctx, st, "k_pt_swap", k_pt_swap<double>, dim3((unsigned)grid), dim3(ASMC_BLOCK), 0, st, n_pairs, par, W, units, lg,
                    (double*)x, ll, lp, c0, c1, betas, k0, k1, round, cnt);
    else
        ASMC_LAUNCH(ctx, st, "k_pt_swap", k_pt_swap<float>, dim3((unsigned)grid), dim3(ASMC_BLOCK), 0, st, n_pairs, par, W, units, lg,
                    (float*)x, ll, lp, c0, c1, betas, k0, k1, round, cnt);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int asmc_pt_evidence(asmc_ctx* ctx, int T, int64_t stride, int64_t offset, int64_t n, const double* ll, const double* coef,
                     double* out, asmc_stream stream) {
    ASMC_REQUIRE(ctx != nullptr && ll != nullptr && coef != nullptr && out != nullptr, "null pointer");
    ASMC_REQUIRE(T >= 1 && T <= ASMC_PT_MAX_RUNGS, "n_temps outside 1 .. ASMC_PT_MAX_RUNGS");
    ASMC_REQUIRE(n > 0 && offset >= 0 && stride > 0 && offset <= stride - n, "the kept samples leave their rung's row");
    // partials [T + 1][gx][4] inside ctx->d_partials (ASMC_MAX_BLOCKS * ASMC_MAX_BETAS * 2 doubles)
    const int gx_cap = (ASMC_MAX_BLOCKS * ASMC_MAX_BETAS * 2) / (4 * (ASMC_PT_MAX_RUNGS + 1));
    const int gx = grid_for(n, ASMC_BLOCK * PT_EV_ITEMS, gx_cap < 1024 ? gx_cap : 1024);
    hipStream_t st = as_stream(stream);
    ASMC_LAUNCH(ctx, st, "k_pt_evidence", k_pt_evidence, dim3(gx, T + 1), dim3(ASMC_BLOCK), 0, st, T, stride, offset, n, ll, coef,
                ctx->d_partials);
    ASMC_LAUNCH_CHECK();
    ASMC_LAUNCH(ctx, st, "k_pt_evidence_final", k_pt_evidence_final, dim3(T + 1), dim3(ASMC_WAVE), 0, st, T, gx,
                (const double*)ctx->d_partials, out);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

}  // extern "C"
