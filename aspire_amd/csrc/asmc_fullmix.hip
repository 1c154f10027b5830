// asmc_fullmix.hip — full-covariance, optionally box-bounded Gaussian mixture: value and per-row gradient in one launch.
//
//   value_i = log sum_c exp(logw_c - 1/2 |W_c (x_i - mu_c)|^2)       W_c lower-triangular, W_c^T W_c = precision of c
//   G_i     = - sum_c resp_c W_c^T (W_c (x_i - mu_c)),                 resp_c = exp(term_c - value_i)
//
// One kernel family, k_fullmix<T, DL, GRAD>, for every 1 <= d <= 128: a row is owned by FOUR adjacent lanes, lane
// s of the quad holding the coordinates j = 4 m + s, m < DL, in registers (D = 4 DL = 4, 8, 16, 32, 64 or 128; narrower d is
// zero-padded).  A block of 256 threads works on tiles of 64 rows: the tile is copied global -> LDS with coalesced loads (16, 8
// or 4 bytes per lane, by the alignment of x: a view that starts at an odd element takes the narrow loads), and each lane picks
// its coordinates out of it.  Row i of the factor is padded to a whole number of quads and read from LDS (four adjacent
// addresses per wave instruction); the quad's partial products are summed over the DPP network (quad_perm), so every lane of the
// quad holds the same v_i bit for bit.  q_c = sum_i v_i^2 in the order of i - with or without the gradient, which is computed
// in a second sweep over the components once the value is known (resp_c needs it), so the value never depends on GRAD.
//
// Components are staged `cg` at a time (all of them when their images fit: always so for d <= 32).  When they do not fit (d > 64,
// or d > 32 with more than four components) the component groups are the OUTER loop over a block's batch of tiles, the running
// (max, sum) of each row waiting in LDS between the passes: an image is staged once per batch, not once per tile.
#include "asmc_common.h"

struct FullMixDev {
    int C, has_bounds;
    const double* logw;
    const double* mu;
    const double* W;
    const double* lo;
    const double* hi;
};

#define FM_BLOCK 256
#define FM_ROWS 64                      // rows of a tile: FM_BLOCK / 4
#define FM_IMG(DL) (8 * (DL) * ((DL) + 1))  // doubles of one component's image: row i holds 4 (i / 4 + 1) entries
#define FM_IMG_BUDGET (72 * 1024)       // bytes of LDS the staged images may take

__host__ __device__ constexpr int fm_row_off(int i) { return 4 * ((i >> 2) + 1) * (2 * (i >> 2) + (i & 3)); }

// sum over the quad's four lanes: lane ^ 1, then lane ^ 2 (a + b == b + a: the four lanes end with the same bits)
template <int CTRL>
__device__ __forceinline__ double fm_quad_move(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)((unsigned long long)b & 0xFFFFFFFFull), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)((unsigned long long)b >> 32), CTRL, 0xF, 0xF, false);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo));
}
#define FM_QUAD_XOR1 0xB1  // quad_perm [1, 0, 3, 2]
#define FM_QUAD_XOR2 0x4E  // quad_perm [2, 3, 0, 1]
__device__ __forceinline__ double fm_quad_sum(double v) {
    v += fm_quad_move<FM_QUAD_XOR1>(v);
    v += fm_quad_move<FM_QUAD_XOR2>(v);
    return v;
}
__device__ __forceinline__ int fm_quad_or(int v) {
    v |= __builtin_amdgcn_update_dpp(0, v, FM_QUAD_XOR1, 0xF, 0xF, false);
    v |= __builtin_amdgcn_update_dpp(0, v, FM_QUAD_XOR2, 0xF, 0xF, false);
    return v;
}

// coalesced copy of the tile's rows global -> LDS by the whole block; bytes behind the last valid row are zero
template <int VEC>
__device__ __forceinline__ void fm_tile_load(const char* __restrict__ g, int64_t valid_bytes, int rowbytes, int ldsrow, char* lds,
                                             int tid) {
    const int tile_bytes = FM_ROWS * rowbytes;
    for (int off = tid * VEC; off < tile_bytes; off += FM_BLOCK * VEC) {
        const int r = off / rowbytes, c = off - r * rowbytes;
        if (VEC == 16) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (off < valid_bytes) v = *reinterpret_cast<const uint4*>(g + off);
            *reinterpret_cast<uint4*>(lds + r * ldsrow + c) = v;
        } else if (VEC == 8) {
            unsigned long long v = 0;
            if (off < valid_bytes) v = *reinterpret_cast<const unsigned long long*>(g + off);
            *reinterpret_cast<unsigned long long*>(lds + r * ldsrow + c) = v;
        } else {
            uint32_t v = 0;
            if (off < valid_bytes) v = *reinterpret_cast<const uint32_t*>(g + off);
            *reinterpret_cast<uint32_t*>(lds + r * ldsrow + c) = v;
        }
    }
}

// q = sum_i v_i^2 with v = W r, row by row (the one sequence behind every value, with or without the gradient)
template <int DL>
__device__ __forceinline__ double fm_quadform(const double* __restrict__ w, int s, const double (&r)[DL]) {
    double q = 0.0;
#pragma unroll
    for (int g = 0; g < DL; g++) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double* __restrict__ wr = w + fm_row_off(4 * g + k) + s;
            double p = 0.0;
#pragma unroll
            for (int mm = 0; mm <= g; mm++) p = fma(wr[4 * mm], r[mm], p);
            const double v = fm_quad_sum(p);
            q = fma(v, v, q);
            // one row of the factor in flight at a time: reads hoisted over more rows cost more registers than the latency they
            // hide
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // a finite row and finite tables give a NaN only where products overflowed to infinities of both signs: the row is too
    // far for fp64, its term is -inf
    return q == q ? q : INFINITY;
}

// ga += nresp * W^T (W r) on the lane's own coordinates: v_i is formed again (the same sequence) and spent at once, so no
// second vector of the row's width waits in registers for the component's responsibility
template <int DL>
__device__ __forceinline__ void fm_grad_acc(const double* __restrict__ w, int s, const double (&r)[DL], double nresp, double (&ga)[DL]) {
#pragma unroll
    for (int g = 0; g < DL; g++) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double* __restrict__ wr = w + fm_row_off(4 * g + k) + s;
            double p = 0.0;
#pragma unroll
            for (int mm = 0; mm <= g; mm++) p = fma(wr[4 * mm], r[mm], p);
            const double sv = nresp * fm_quad_sum(p);
#pragma unroll
            for (int mm = 0; mm <= g; mm++) ga[mm] = fma(wr[4 * mm], sv, ga[mm]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

template <typename T, int DL, bool GRAD>
__global__ __launch_bounds__(FM_BLOCK, (DL <= 4 ? 4 : DL <= 16 ? 2 : 1)) void k_fullmix(int64_t n, int d, const T* __restrict__ x, FullMixDev m, double* __restrict__ out,
                                                     double* __restrict__ grad, int cg, int bt, int ldsrow, int vec) {
    constexpr int D = 4 * DL;
    constexpr int IMG = FM_IMG(DL);
    extern __shared__ __align__(16) char smem[];
    double* s_w = reinterpret_cast<double*>(smem);  // [cg][IMG]
    double* s_mu = s_w + (size_t)cg * IMG;           // [cg][D]
    double* s_lo = s_mu + cg * D;                    // [D]
    double* s_hi = s_lo + D;                         // [D]
    double* s_logw = s_hi + D;                       // [ASMC_MAX_COMPONENTS]
    double* s_max = s_logw + ASMC_MAX_COMPONENTS;    // [bt * 64] running max; the value once the last group is through
    double* s_sum = s_max + bt * FM_ROWS;            // [bt * 64] running sum
    int* s_cls = reinterpret_cast<int*>(s_sum + bt * FM_ROWS);  // [bt * 64] 0 finite and inside the box, 1 NaN, 2 -inf
    char* s_x = reinterpret_cast<char*>(s_cls + bt * FM_ROWS);  // [64][ldsrow]

    const int tid = threadIdx.x, s = tid & 3, rl = tid >> 2;
    const int C = m.C;
    const int rowbytes = d * (int)sizeof(T);
    const int64_t n_tiles = (n + FM_ROWS - 1) / FM_ROWS, n_batches = (n_tiles + bt - 1) / bt;
    const bool single = C <= cg;  // every component staged at once: staged once per block, tile loop outermost
    for (int e = tid; e < D; e += FM_BLOCK) {
        s_lo[e] = (m.has_bounds && e < d) ? m.lo[e] : -INFINITY;
        s_hi[e] = (m.has_bounds && e < d) ? m.hi[e] : INFINITY;
    }
    if (tid < ASMC_MAX_COMPONENTS) s_logw[tid] = tid < C ? m.logw[tid] : -INFINITY;
    bool staged = false;
    const T* xrow = reinterpret_cast<const T*>(s_x + rl * ldsrow);

    for (int64_t batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
        const int64_t t0 = batch * bt, t1 = (t0 + bt < n_tiles) ? t0 + bt : n_tiles;
#pragma unroll 1
        for (int sweep = 0; sweep < (GRAD ? 2 : 1); sweep++) {
#pragma unroll 1
            for (int c0 = 0; c0 < C; c0 += cg) {
                const int ng = (C - c0 < cg) ? C - c0 : cg;
                if (!(single && staged)) {
                    __syncthreads();  // the images' last readers are through
                    for (int e = tid; e < ng * D * D; e += FM_BLOCK) {
                        const int c = e / (D * D), i = (e / D) % D, j = e % D;
                        if (j < 4 * ((i >> 2) + 1))
                            s_w[(size_t)c * IMG + fm_row_off(i) + j] =
                                (i < d && j <= i) ? m.W[((size_t)(c0 + c) * d + i) * d + j] : 0.0;
                    }
                    for (int e = tid; e < ng * D; e += FM_BLOCK) {
                        const int c = e / D, j = e % D;
                        s_mu[e] = j < d ? m.mu[(size_t)(c0 + c) * d + j] : 0.0;
                    }
                    staged = true;
                }
#pragma unroll 1
                for (int64_t t = t0; t < t1; t++) {
                    const bool resident = GRAD && sweep == 1 && single && t1 - t0 == 1;  // the value sweep left this tile in LDS
                    if (!resident) {
                        __syncthreads();  // the tile's last readers are through
                        const int64_t rows = (n - t * FM_ROWS < FM_ROWS) ? n - t * FM_ROWS : FM_ROWS;
                        const char* gb = reinterpret_cast<const char*>(x) + t * FM_ROWS * (int64_t)rowbytes;
                        if (vec == 16) fm_tile_load<16>(gb, rows * rowbytes, rowbytes, ldsrow, s_x, tid);
                        else if (vec == 8) fm_tile_load<8>(gb, rows * rowbytes, rowbytes, ldsrow, s_x, tid);
                        else fm_tile_load<4>(gb, rows * rowbytes, rowbytes, ldsrow, s_x, tid);
                    }
                    __syncthreads();
                    const int64_t row = t * FM_ROWS + rl;
                    const bool live = row < n;
                    const int slot = (int)(t - t0) * FM_ROWS + rl;
                    int cls;
                    if (sweep == 0 && c0 == 0) {  // the explicit test of the row: NaN first, then +-inf and the box
                        int f = 0;
#pragma unroll
                        for (int mm = 0; mm < DL; mm++) {
                            const int j = 4 * mm + s;
                            if (j < d) {
                                const double v = (double)xrow[j];
                                if (v != v) f |= 1;
                                else if (isinf(v) || v < s_lo[j] || v > s_hi[j]) f |= 2;
                            }
                        }
                        f = fm_quad_or(f);
                        cls = (f & 1) ? 1 : (f ? 2 : 0);
                        if (s == 0) s_cls[slot] = cls;
                    } else {
                        cls = s_cls[slot];
                    }
                    const bool plain = live && cls == 0;  // any other row runs the arithmetic on zeros
                    if (sweep == 0) {
                        double M = -INFINITY, S = 0.0;
                        if (c0 > 0) {
                            M = s_max[slot];
                            S = s_sum[slot];
                        }
#pragma unroll 1
                        for (int c = 0; c < ng; c++) {
                            double r[DL];
#pragma unroll
                            for (int mm = 0; mm < DL; mm++) {
                                const int j = 4 * mm + s;
                                r[mm] = ((j < d && plain) ? (double)xrow[j] : 0.0) - ((j < d && plain) ? s_mu[c * D + j] : 0.0);
                            }
                            const double q = fm_quadform<DL>(s_w + (size_t)c * IMG, s, r);
                            const double term = s_logw[c0 + c] - 0.5 * q;
                            if (term > M) {
                                S = fma(S, exp(M - term), 1.0);
                                M = term;
                            } else if (term > -INFINITY) {
                                S += exp(term - M);
                            }
                        }
                        if (c0 + ng >= C) {
                            double val = (M == -INFINITY) ? -INFINITY : M + log(S);
                            if (cls == 1) val = __longlong_as_double(0x7FF8000000000000LL);
                            else if (cls == 2) val = -INFINITY;
                            if (s == 0) {
                                if (live) out[row] = val;
                                if (GRAD) s_max[slot] = val;
                            }
                        } else if (s == 0) {
                            s_max[slot] = M;
                            s_sum[slot] = S;
                        }
                    } else {
                        const double val = s_max[slot];
                        const bool ok = plain && val > -INFINITY && val < INFINITY;
                        double ga[DL];
#pragma unroll
                        for (int mm = 0; mm < DL; mm++) {
                            const int j = 4 * mm + s;
                            ga[mm] = (c0 > 0 && live && j < d) ? grad[row * d + j] : 0.0;
                        }
#pragma unroll 1
                        for (int c = 0; c < ng; c++) {
                            double r[DL];
#pragma unroll
                            for (int mm = 0; mm < DL; mm++) {
                                const int j = 4 * mm + s;
                                r[mm] = ((j < d && plain) ? (double)xrow[j] : 0.0) - ((j < d && plain) ? s_mu[c * D + j] : 0.0);
                            }
                            const double q = fm_quadform<DL>(s_w + (size_t)c * IMG, s, r);
                            const double term = s_logw[c0 + c] - 0.5 * q;
                            const double resp = ok ? exp(term - val) : 0.0;
                            // the residual is read again through a volatile pointer: the second pass over the factor must
                            // form its v_i afresh and not keep the first pass's D of them alive in every lane (hipcc otherwise
                            // merges the two passes' identical chains).  What to check after a compiler change, from
                            // -Rpass-analysis=kernel-resource-usage of the GRAD instantiations (when written: DL = 8: 255 registers,
                            // no scratch, two waves per SIMD; DL = 16: 256 registers, 596 bytes of scratch per lane; DL = 32: 256,
                            // 1188 bytes): scratch far beyond these means the passes were merged again.  The price is DL more
                            // LDS reads per component and row, next to the D (D + 1) / 8 of the factor.
                            const volatile double* vmu = s_mu + c * D;
#pragma unroll
                            for (int mm = 0; mm < DL; mm++) {
                                const int j = 4 * mm + s;
                                r[mm] = ((j < d && plain) ? (double)xrow[j] : 0.0) - ((j < d && plain) ? vmu[j] : 0.0);
                            }
                            fm_grad_acc<DL>(s_w + (size_t)c * IMG, s, r, -resp, ga);
                        }
                        if (live) {
#pragma unroll
                            for (int mm = 0; mm < DL; mm++) {
                                const int j = 4 * mm + s;
                                if (j < d) grad[row * d + j] = ok ? ga[mm] : 0.0;  // a non-finite value: an all-zero row, never NaN
                            }
                        }
                    }
                }
            }
        }
    }
}

static int fm_lds_row(int rowbytes, int elem) {
    // a quad reads 4 adjacent elements, a wave 16 rows: the stride that spreads a lane group's rows over all banks is 32 bytes
    // past a multiple of 256 for fp64 rows (ds_read_b64: 64 banks, 32 lanes), 16 past a multiple of 128 for fp32 rows
    int s = (rowbytes + 15) & ~15;
    const int mod = elem == 8 ? 256 : 128, rem = elem == 8 ? 32 : 16;
    while (s % mod != rem) s += 16;
    return s;
}

template <typename T, int DL>
static int fm_launch(asmc_ctx* ctx, int64_t n, int d, const T* x, const FullMixDev& m, double* out, double* grad, hipStream_t st) {
    constexpr int D = 4 * DL;
    const int img_bytes = FM_IMG(DL) * 8;
    int cg = FM_IMG_BUDGET / img_bytes;
    if (cg < 1) cg = 1;
    if (cg > m.C) cg = m.C;
    const int bt = m.C <= cg ? 1 : 8;
    const int rowbytes = d * (int)sizeof(T);
    const int ldsrow = fm_lds_row(rowbytes, (int)sizeof(T));
    const uintptr_t a = (uintptr_t)x;
    const int vec = (rowbytes % 16 == 0 && a % 16 == 0) ? 16 : (rowbytes % 8 == 0 && a % 8 == 0) ? 8 : 4;
    const size_t lds = (size_t)cg * img_bytes + 8 * ((size_t)cg * D + 2 * D + ASMC_MAX_COMPONENTS) + (size_t)bt * FM_ROWS * 20 +
                       (size_t)FM_ROWS * ldsrow;
    if (lds > 160 * 1024) {
        asmc_set_error("asmc_fullmix_logpdf: tables exceed the LDS");
        return ASMC_ERR_UNSUPPORTED;
    }
    const int64_t n_tiles = (n + FM_ROWS - 1) / FM_ROWS, n_batches = (n_tiles + bt - 1) / bt;
    const int grid = grid_for(n_batches, 1, ctx->num_cu * 4);
    auto go = [&](auto kern) {
        if (lds > 64 * 1024)
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        ASMC_LAUNCH(ctx, st, "k_fullmix", kern, dim3(grid), dim3(FM_BLOCK), lds, st, n, d, x, m, out, grad, cg, bt, ldsrow, vec);
    };
    if (grad) go(k_fullmix<T, DL, true>);
    else go(k_fullmix<T, DL, false>);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

template <typename T>
static int fm_dispatch(asmc_ctx* ctx, int64_t n, int d, const void* x, const FullMixDev& m, double* out, double* grad, hipStream_t st) {
    const T* xp = reinterpret_cast<const T*>(x);
    if (d <= 4) return fm_launch<T, 1>(ctx, n, d, xp, m, out, grad, st);
    if (d <= 8) return fm_launch<T, 2>(ctx, n, d, xp, m, out, grad, st);
    if (d <= 16) return fm_launch<T, 4>(ctx, n, d, xp, m, out, grad, st);
    if (d <= 32) return fm_launch<T, 8>(ctx, n, d, xp, m, out, grad, st);
    if (d <= 64) return fm_launch<T, 16>(ctx, n, d, xp, m, out, grad, st);
    return fm_launch<T, 32>(ctx, n, d, xp, m, out, grad, st);
}

extern "C" {

int asmc_fullmix_logpdf(asmc_ctx* ctx, int64_t n, int d, int x_dtype, const void* x, const asmc_fullmix* density, double* out,
                        double* grad, asmc_stream stream) {
    ASMC_REQUIRE(ctx && x && density && out, "null pointer");
    ASMC_REQUIRE(n > 0, "bad sizes");
    ASMC_REQUIRE(x_dtype == ASMC_F64 || x_dtype == ASMC_F32, "bad x_dtype");
    ASMC_REQUIRE(density->logw_dev && density->mu_dev && density->whiten_dev, "null device pointer");
    ASMC_REQUIRE(!density->has_bounds || (density->lower_dev && density->upper_dev), "bounds without tables");
    const int elem = x_dtype == ASMC_F64 ? 8 : 4;
    if (d < 1 || d > 128 || density->n_components < 1 || density->n_components > ASMC_MAX_COMPONENTS || (uintptr_t)x % elem != 0) {
        asmc_set_error("asmc_fullmix_logpdf: 1 <= d <= 128, 1 <= components <= %d, element-aligned rows", ASMC_MAX_COMPONENTS);
        return ASMC_ERR_UNSUPPORTED;
    }
    const FullMixDev m = {density->n_components, density->has_bounds, density->logw_dev, density->mu_dev, density->whiten_dev,
                          density->lower_dev, density->upper_dev};
    hipStream_t st = as_stream(stream);
    if (x_dtype == ASMC_F64) return fm_dispatch<double>(ctx, n, d, x, m, out, grad, st);
    return fm_dispatch<float>(ctx, n, d, x, m, out, grad, st);
}

}  // extern "C"
