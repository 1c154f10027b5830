// asmc_moments.hip — population moments (column sums, centred Gram matrix) and the reference-fit factorisation.
#include <stdlib.h>

#include "asmc_pcn_shared.h"

// =============================================================================================
// population moments
// =============================================================================================
template <typename T>
__global__ __launch_bounds__(ASMC_BLOCK) void k_colsum(int64_t n, int d, const T* __restrict__ x,
                                                      double* __restrict__ partials) {
    // thread t owns column (t % d) when ASMC_BLOCK % d == 0, otherwise a strided element walk with
    // per-element column lookup; partial sums are combined through LDS atomics-free reduction.
    extern __shared__ __align__(16) char smem[];
    double* s_acc = reinterpret_cast<double*>(smem);  // [ASMC_BLOCK]
    const int rows_per_pass = ASMC_BLOCK / d;         // >= 1 (d <= 256)
    const int my_col = threadIdx.x % d;
    const int my_sub = threadIdx.x / d;
    double acc = 0.0;
    if (my_sub < rows_per_pass) {
        for (int64_t r = (int64_t)blockIdx.x * rows_per_pass + my_sub; r < n; r += (int64_t)gridDim.x * rows_per_pass)
            acc += (double)x[r * d + my_col];
    }
    s_acc[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x < d) {
        double v = 0.0;
        for (int s = 0; s < rows_per_pass; s++) v += s_acc[s * d + threadIdx.x];
        partials[(size_t)blockIdx.x * d + threadIdx.x] = v;
    }
}

// gram partial: G[j,k] += (x_ij - c_j)(x_ik - c_k) over the block's rows; tile of 64 centred rows in LDS
template <typename T>
__global__ __launch_bounds__(ASMC_BLOCK) void k_gram(int64_t n, int d, const T* __restrict__ x,
                                                    const double* __restrict__ center,
                                                    double* __restrict__ partials) {
    extern __shared__ __align__(16) char smem[];
    double* s_rows = reinterpret_cast<double*>(smem);  // [64][d+1]
    const int ld = d + 1;
    const int dd = d * d;
    // entries e = tid, tid+256, ... (< d*d <= 4096): at most 16 accumulators per thread
    double acc[16];
    int jj[16], kk[16];
#pragma unroll
    for (int a = 0; a < 16; a++) {
        acc[a] = 0.0;
        const int e = threadIdx.x + a * ASMC_BLOCK;
        const int ec = e < dd ? e : 0;
        jj[a] = ec / d;
        kk[a] = ec - jj[a] * d;
    }
    for (int64_t row0 = (int64_t)blockIdx.x * 64; row0 < n; row0 += (int64_t)gridDim.x * 64) {
        __syncthreads();
        for (int e = threadIdx.x; e < 64 * d; e += ASMC_BLOCK) {
            const int r = e / d, c = e - r * d;
            const int64_t gr = row0 + r;
            s_rows[r * ld + c] = gr < n ? (double)x[gr * d + c] - center[c] : 0.0;
        }
        __syncthreads();
#pragma unroll 2
        for (int r = 0; r < 64; r++) {
            const double* row = s_rows + r * ld;
#pragma unroll
            for (int a = 0; a < 16; a++)
                if (a * ASMC_BLOCK < dd) acc[a] = fma(row[jj[a]], row[kk[a]], acc[a]);
        }
    }
#pragma unroll
    for (int a = 0; a < 16; a++) {
        const int e = threadIdx.x + a * ASMC_BLOCK;
        if (e < dd) partials[(size_t)blockIdx.x * dd + e] = acc[a];
    }
}

// Register-blocked centred Gram matrix: one wave owns a (8*BLK) x (8*BLK) quadrant of G, lane (bi, bj) a
// BLK x BLK block of it (16 or 64 accumulators in VGPRs).  Rows are staged 64 at a time through the wave's
// LDS tile with coalesced 16-B loads; per row every lane reads two BLK-wide slices (same row for all lanes:
// LDS broadcast, conflict free) and issues BLK^2 FMAs — 0.5 (BLK=4) / 0.25 (BLK=8) LDS reads per FMA.
// blockIdx.y selects the quadrant (d > 8*BLK needs several).  Block partial [d_pad x d_pad] per block.
template <typename T, int BLK>
__global__ __launch_bounds__(ASMC_BLOCK) void k_gram_rb(int64_t n, int d, const T* __restrict__ x,
                                                       const double* __restrict__ center,
                                                       double* __restrict__ partials, int n_quad_side) {
    extern __shared__ __align__(16) char smem[];
    constexpr int Q = 8 * BLK;  // quadrant side
    const int rowbytes = d * (int)sizeof(T);
    const int ldsrow = lds_row_stride(rowbytes);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    char* tile = smem + (size_t)wave * 64 * ldsrow;
    const int qi = blockIdx.y / n_quad_side, qj = blockIdx.y % n_quad_side;
    const int bi = lane >> 3, bj = lane & 7;
    const int i0 = qi * Q + bi * BLK, j0 = qj * Q + bj * BLK;  // first row / column of this lane's block
    double ci[BLK], cj[BLK], acc[BLK][BLK];
#pragma unroll
    for (int a = 0; a < BLK; a++) {
        ci[a] = (i0 + a < d) ? center[i0 + a] : 0.0;
        cj[a] = (j0 + a < d) ? center[j0 + a] : 0.0;
#pragma unroll
        for (int b = 0; b < BLK; b++) acc[a][b] = 0.0;
    }
    const int64_t n_tiles = (n + 63) / 64;
    const int wpb = (int)(blockDim.x >> 6);
    for (int64_t t = (int64_t)blockIdx.x * wpb + wave; t < n_tiles; t += (int64_t)gridDim.x * wpb) {
        const int64_t row0 = t * 64;
        const int rows = (int)((n - row0) < 64 ? (n - row0) : 64);
        wave_lds_sync();
        tile_load<16>(reinterpret_cast<const char*>(x) + row0 * rowbytes, (int64_t)rows * rowbytes, rowbytes, ldsrow, tile, lane);
        wave_lds_sync();
        for (int r = 0; r < rows; r++) {
            const T* row = reinterpret_cast<const T*>(tile + r * ldsrow);
            double ai[BLK], aj[BLK];
#pragma unroll
            for (int a = 0; a < BLK; a++) {
                ai[a] = (i0 + a < d) ? (double)row[i0 + a] - ci[a] : 0.0;
                aj[a] = (j0 + a < d) ? (double)row[j0 + a] - cj[a] : 0.0;
            }
#pragma unroll
            for (int a = 0; a < BLK; a++)
#pragma unroll
                for (int b = 0; b < BLK; b++) acc[a][b] = fma(ai[a], aj[b], acc[a][b]);
        }
    }
    // combine the block's waves through LDS (fixed order), write the block partial of this quadrant
    __syncthreads();
    double* red = reinterpret_cast<double*>(smem);  // [wpb][Q*Q] fits: Q*Q*8 <= 64*ldsrow for d >= Q/2
    double* mine = red + (size_t)wave * Q * Q;
#pragma unroll
    for (int a = 0; a < BLK; a++)
#pragma unroll
        for (int b = 0; b < BLK; b++) mine[(bi * BLK + a) * Q + bj * BLK + b] = acc[a][b];
    __syncthreads();
    const int dpad = n_quad_side * Q;
    for (int e = threadIdx.x; e < Q * Q; e += (int)blockDim.x) {
        double v = red[e];
        for (int w = 1; w < wpb; w++) v += red[(size_t)w * Q * Q + e];
        const int gi = qi * Q + e / Q, gj = qj * Q + e % Q;
        partials[(size_t)blockIdx.x * dpad * dpad + (size_t)gi * dpad + gj] = v;
    }
}

// one block per column; 64 threads (one wave: the order every caller has always had) or 256 (the gather's column-sum partials:
// 4 096 rows - 24 us with one wave): strided partial sums, the wave's butterfly, then the waves in order
// keep / center (optional): the sum also goes to keep[col] (the copy asmc_reference_factor reads in ctx->d_ref) and
// center[col] = sum / n_mean (k_center_from_sum's division)
__global__ __launch_bounds__(256) void k_reduce_columns(int nblocks, int ncols, const double* __restrict__ partials,
                                                       double* __restrict__ out, double* __restrict__ keep = nullptr,
                                                       double* __restrict__ center = nullptr, double n_mean = 1.0) {
    __shared__ double s_w[4];
    const int nt = (int)blockDim.x;
    for (int col = blockIdx.x; col < ncols; col += gridDim.x) {
        double v = 0.0;
        for (int b = threadIdx.x; b < nblocks; b += nt) v += partials[(size_t)b * ncols + col];
        v = wave_sum(v);
        if (nt != 64) {
            if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
            __syncthreads();
            v = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            out[col] = v;
            if (keep) keep[col] = v;
            if (center) center[col] = v / n_mean;
        }
    }
}

extern "C" {

int asmc_colsum(asmc_ctx* ctx, int64_t n, int d, int x_dtype, const void* x, double* sum_host, asmc_stream stream) {
    ASMC_REQUIRE(ctx && x && sum_host, "null pointer");
    ASMC_REQUIRE(n > 0 && d > 0 && d <= ctx->d_max && d <= ASMC_BLOCK, "bad sizes");
    ASMC_REQUIRE(x_dtype == ASMC_F64 || x_dtype == ASMC_F32, "bad x_dtype");
    hipStream_t st = as_stream(stream);
    int grid = grid_for(n, (ASMC_BLOCK / d) * 16, ctx->gram_blocks);
    if (x_dtype == ASMC_F64)
        ASMC_LAUNCH(ctx, st, "k_colsum<double>", k_colsum<double>, dim3(grid), dim3(ASMC_BLOCK), ASMC_BLOCK * sizeof(double), st, n, d, (const double*)x, ctx->d_gram);
    else
        ASMC_LAUNCH(ctx, st, "k_colsum<float>", k_colsum<float>, dim3(grid), dim3(ASMC_BLOCK), ASMC_BLOCK * sizeof(double), st, n, d, (const float*)x, ctx->d_gram);
    ASMC_LAUNCH_CHECK();
    ASMC_LAUNCH(ctx, st, "k_reduce_columns", k_reduce_columns, dim3(d), dim3(64), 0, st, grid, d, (const double*)ctx->d_gram, ctx->d_small);
    ASMC_LAUNCH_CHECK();
    ASMC_HIP(hipMemcpyAsync(ctx->h_pinned, ctx->d_small, sizeof(double) * d, hipMemcpyDeviceToHost, st));
    ASMC_HIP(hipStreamSynchronize(st));
    memcpy(sum_host, ctx->h_pinned, sizeof(double) * d);
    return ASMC_OK;
}

__global__ void k_center_from_sum(int d, const double* __restrict__ sum, double n, double* __restrict__ center) {
    const int j = threadIdx.x;
    if (j < d) center[j] = sum[j] / n;
}

// The reference Gaussian of a mutation from the population moments, on the device (smc/minipcn.py:75-84: mean and
// covariance of the particles; this repository's pCN specification whitens with the Cholesky factor): what the host did with
// numpy between two temperatures - cov = G / (n - 1), symmetrised; L = chol(cov + jitter * mean(diag) * I) with the jitter
// ladder 0, 1e-12, 1e-10, ... of twelve tries (denom = n - 1); Linv = L^-1 - in ONE block behind the Gram kernel, so the mutation's kernels
// follow without a host round trip (fetch, LAPACK, upload: ~0.2 ms of idle GPU per temperature).
// out = [mu (seg) | L (d x d, zeros above the diagonal) | pad to seg x d | Linv (d x d)], seg = 32 ceil(d / 32) doubles;
// status[0] = jitter tries used (0: none), -1: not factorable / not finite.
#define REF_THREADS 256
// Also the factorisation inside the device-side EM of the Student-t reference (asmc_student_fit): `sum` == NULL leaves the mean
// alone, `tab` (mu | Linv's lower triangle packed by rows) is what k_student_estep stages, `em` / `it`: the EM's state record -
// iterations behind the one that converged are skipped, a failed factorisation is recorded there.
__global__ __launch_bounds__(1024) void k_ref_factor(int d, const double* __restrict__ sum, const double* __restrict__ gram,
                                                           double n_mean, double denom, double* __restrict__ out,
                                                           double* __restrict__ status, double* __restrict__ tab,
                                                           double* __restrict__ em, int it) {
    extern __shared__ __align__(16) double s_a[];  // [d][d + 1]
    __shared__ double s_diag[128], s_rdiag[128];
    __shared__ double s_scale;
    if (em && (double)it > em[2]) return;  // (uniform: every thread reads the same cell)
    const int tid = threadIdx.x, ld = d + 1, seg = (d + 31) / 32 * 32;
    const int NT = (int)blockDim.x;  // (one wave for d <= 32 - free barriers - was measured: 63 us against 40 with four)
    double* o_mu = out;
    double* o_L = out + seg;
    double* o_Li = out + seg + (size_t)seg * d;
    if (sum)
        for (int j = tid; j < d; j += NT) {
            const double mj = sum[j] / n_mean;
            if (out) o_mu[j] = mj;
            if (tab) tab[j] = mj;
        }
    const double inv_denom = 1.0 / denom;
    int tries = -1;
    double jitter = 0.0;
    for (int attempt = 0; attempt < 12; attempt++) {
        __syncthreads();
        for (int e = tid; e < d * d; e += NT) {
            const int i = e / d, j = e - i * d;
            s_a[i * ld + j] = 0.5 * (gram[(size_t)i * d + j] * inv_denom + gram[(size_t)j * d + i] * inv_denom);
        }
        __syncthreads();
        if (attempt == 0) {
            if (tid == 0) {
                double t = 0.0;
                for (int j = 0; j < d; j++) t += s_a[j * ld + j];
                t /= (double)d;
                s_scale = (t > 0.0 && t < INFINITY) ? t : 1.0;
            }
        } else {
            for (int j = tid; j < d; j += NT) s_a[j * ld + j] += jitter * s_scale;
        }
        // right-looking Cholesky with ONE barrier per column: the trailing block takes A[i][k] -= A[i][j] A[k][j] / A[j][j]
        // (kept symmetric: both halves are updated); column j itself is left unscaled - it is not read again - and becomes
        // L[i][j] = A[i][j] / sqrt(A[j][j]) in the pass behind the loop
        bool ok = true;
        for (int j = 0; j < d; j++) {
            __syncthreads();
            const double p = s_a[j * ld + j];  // the same value in every thread: the test below is uniform
            if (!(p > 0.0 && p < INFINITY)) {
                ok = false;
                break;
            }
            double rp = __builtin_amdgcn_rcp(p);  // hardware reciprocal + two Newton steps: the division's chain is half of a column's latency
            rp = fma(fma(-p, rp, 1.0), rp, rp);
            rp = fma(fma(-p, rp, 1.0), rp, rp);
            // threads as a (NT / 32) x 32 patch walking the trailing block: no integer division per element
            for (int i = j + 1 + (tid >> 5); i < d; i += NT >> 5) {
                const double li = s_a[i * ld + j] * rp;
                for (int k = j + 1 + (tid & 31); k < d; k += 32) s_a[i * ld + k] = fma(-li, s_a[k * ld + j], s_a[i * ld + k]);
            }
        }
        if (ok) {
            tries = attempt;
            break;
        }
        jitter = jitter == 0.0 ? 1e-12 : jitter * 100.0;
    }
    __syncthreads();
    if (tid == 0) {
        if (status) status[0] = (double)tries;
        if (em && tries < 0) em[3] = -1.0;
    }
    if (tries < 0) {
        // no factor: poison (L, Linv) so that a mutation that runs before the host has looked at the status cannot use the
        // factors an earlier fit left in this slot - NaN proposals are rejected and counted, never silently accepted
        if (out)
            for (int e = tid; e < d * d; e += NT) o_L[e] = __builtin_nan(""), o_Li[e] = __builtin_nan("");
        if (tab)
            for (int e = tid; e < d * (d + 1) / 2; e += NT) tab[d + e] = __builtin_nan("");
        return;
    }
    for (int j = tid; j < d; j += NT) {
        const double sd = sqrt(s_a[j * ld + j]);
        s_diag[j] = sd, s_rdiag[j] = 1.0 / sd;
    }
    __syncthreads();
    for (int e = tid; e < d * d; e += NT) {
        const int i = e / d, j = e - i * d;
        double v = 0.0;
        if (j < i) v = s_a[i * ld + j] * s_rdiag[j];
        if (j == i) v = s_diag[j];
        if (out) o_L[e] = v;
        if (j < i) s_a[i * ld + j] = v;  // (the strict lower triangle: no other thread touches it in this pass)
    }
    __syncthreads();
    // Linv by forward substitution, every column at once and without a block barrier: a group of G lanes of one wave solves
    // L x = e_c for column c - the lanes split the dot product of a row (a single lane's chain of d^2 / 2 dependent LDS reads
    // was 30 of the kernel's 40 us at d = 32 and 520 us at d = 128) - and keeps x_i (i > c) in the FREE upper triangle, at
    // A[c][i], its own row; L is only read.  LDS operations of a wave complete in order: the lanes of a group see x_i
    // as soon as the instruction that wrote it has issued.
    {
        const int per = NT / d;
        const int G = per >= 8 ? 8 : per >= 4 ? 4 : per >= 2 ? 2 : 1;
        const int c = tid / G, q = tid % G;
        if (c < d) {
            const double xc = s_rdiag[c];
            for (int i = c + 1; i < d; i++) {
                double acc = q == 0 ? s_a[i * ld + c] * xc : 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
                int k = c + 1 + q;
                for (; k + 3 * G < i; k += 4 * G) {  // four independent chains: the LDS reads of a row pipeline
                    acc = fma(s_a[i * ld + k], s_a[c * ld + k], acc);
                    acc1 = fma(s_a[i * ld + k + G], s_a[c * ld + k + G], acc1);
                    acc2 = fma(s_a[i * ld + k + 2 * G], s_a[c * ld + k + 2 * G], acc2);
                    acc3 = fma(s_a[i * ld + k + 3 * G], s_a[c * ld + k + 3 * G], acc3);
                }
                for (; k < i; k += G) acc = fma(s_a[i * ld + k], s_a[c * ld + k], acc);
                acc = (acc + acc1) + (acc2 + acc3);
                for (int o = G >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
                if (q == 0) s_a[c * ld + i] = -acc * s_rdiag[i];
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < d * d; e += NT) {
        const int i = e / d, j = e - i * d;
        const double v = j < i ? s_a[j * ld + i] : j == i ? s_rdiag[i] : 0.0;
        if (out) o_Li[e] = v;
        if (tab && j <= i) tab[d + i * (i + 1) / 2 + j] = v;
    }
}

// Column sums and the Gram matrix centred on sum / n_mean in ONE enqueue and one synchronisation (the reference fit of a
// temperature boundary: the centre never visits the host; same division, same kernels, same bits as asmc_colsum -> host
// division -> asmc_centered_gram).  _enqueue leaves both results on their way to pinned memory, _fetch waits for the stream
// and hands them out: a caller with other work on the stream (the importance step's chain) pays one synchronisation for all.
int asmc_mean_gram_enqueue(asmc_ctx* ctx, int64_t n, int d, int x_dtype, const void* x, int64_t n_mean, int across_flags,
                           asmc_stream stream) {
    const int across_ranks = across_flags & ASMC_GRAM_ACROSS_RANKS;
    ASMC_REQUIRE(ctx && x, "null pointer");
    ASMC_REQUIRE(n > 0 && n_mean > 0 && d > 0 && d <= ctx->d_max && d <= 128, "bad sizes (gram supports d <= 128)");
    ASMC_REQUIRE(x_dtype == ASMC_F64 || x_dtype == ASMC_F32, "bad x_dtype");
    ASMC_REQUIRE(asmc_gram_mm_supported(d, x) && d <= ASMC_BLOCK && !getenv("ASMC_GRAM_GENERIC"),
                 "shape without the device-side path (asmc_mean_gram falls back to the two calls; across_ranks: merge on the host)");
    typedef int (*allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
    const allreduce_fn allreduce = reinterpret_cast<allreduce_fn>(ctx->rccl_allreduce);
    const int nccl_f64 = 8, nccl_sum = 0;  // rccl.h: ncclFloat64, ncclSum
    ASMC_REQUIRE(!across_ranks || (allreduce && ctx->rccl_comm), "across_ranks needs asmc_set_rccl");
    hipStream_t st = as_stream(stream);
    int grid = grid_for(n, (ASMC_BLOCK / d) * 16, ctx->gram_blocks);
    // rows that asmc_gather has just written AND that the caller vouches for (ASMC_GRAM_FROM_GATHER: nothing has rewritten them
    // since - the library cannot see a caller's own kernels): their column-sum partials came with the gather, no pass over the rows
    const bool from_gather = (across_flags & ASMC_GRAM_FROM_GATHER) && ctx->cs_n == n && ctx->cs_x == x && ctx->cs_d == d &&
                             x_dtype == ASMC_F64;
    if (from_gather)
        grid = ctx->cs_grid;
    else if (x_dtype == ASMC_F64)
        ASMC_LAUNCH(ctx, st, "k_colsum<double>", k_colsum<double>, dim3(grid), dim3(ASMC_BLOCK), ASMC_BLOCK * sizeof(double), st, n, d, (const double*)x, ctx->d_gram);
    else
        ASMC_LAUNCH(ctx, st, "k_colsum<float>", k_colsum<float>, dim3(grid), dim3(ASMC_BLOCK), ASMC_BLOCK * sizeof(double), st, n, d, (const float*)x, ctx->d_gram);
    ASMC_LAUNCH_CHECK();
    // the results stay on the device in ctx->d_ref = {sums [128], Gram} (d_small / d_partials are every call's scratch):
    // asmc_reference_factor reads them there, asmc_mean_gram_fetch copies them out when a caller wants them on the host.  The
    // reductions write them there themselves, the all-reduces of a sharded run work on them in place, and the Gram kernel forms
    // the centre sum / n_mean itself: no launch sits between the passes and the collectives.
    ASMC_LAUNCH(ctx, st, "k_reduce_columns", k_reduce_columns, dim3(d), dim3(from_gather ? 256 : 64), 0, st, grid, d,
                (const double*)ctx->d_gram, ctx->d_small, ctx->d_ref, (double*)nullptr, (double)n_mean);
    ASMC_LAUNCH_CHECK();
    if (across_ranks && allreduce(ctx->d_ref, ctx->d_ref, (size_t)d, nccl_f64, nccl_sum, ctx->rccl_comm, st) != 0) {
        asmc_set_error("asmc_mean_gram: ncclAllReduce failed");
        return ASMC_ERR_ARG;
    }
    int ggrid = 0;
    int rc = asmc_gram_mm_launch(ctx, n, d, x_dtype, x, ctx->d_ref, &ggrid, st, ctx->d_ref + 128, (double)n_mean);
    if (rc) return rc;
    if (across_ranks && allreduce(ctx->d_ref + 128, ctx->d_ref + 128, (size_t)d * d, nccl_f64, nccl_sum, ctx->rccl_comm, st) != 0) {
        asmc_set_error("asmc_mean_gram: ncclAllReduce failed");
        return ASMC_ERR_ARG;
    }
    ctx->gram_pending_d = d;
    return ASMC_OK;
}

int asmc_mean_gram_fetch(asmc_ctx* ctx, int d, double* sum_host, double* gram_host, asmc_stream stream) {
    ASMC_REQUIRE(ctx && sum_host && gram_host, "null pointer");
    ASMC_REQUIRE(ctx->gram_pending_d == d && d > 0, "no asmc_mean_gram_enqueue of this d is pending");
    ASMC_HIP(hipMemcpyAsync(ctx->h_gram, ctx->d_ref, sizeof(double) * (128 + (size_t)d * d), hipMemcpyDeviceToHost, as_stream(stream)));
    ASMC_HIP(hipStreamSynchronize(as_stream(stream)));
    memcpy(sum_host, ctx->h_gram, sizeof(double) * d);
    memcpy(gram_host, ctx->h_gram + 128, sizeof(double) * d * d);
    ctx->gram_pending_d = 0;
    return ASMC_OK;
}

}  // extern "C"
// Every factorisation request reads its status back into a pinned cell OF ITS OWN (a ring indexed by a generation counter): the
// host writes the "not yet known" sentinel into a cell that no copy still in flight targets - an earlier request's late copy
// lands in its own cell and cannot be mistaken for this request's status.  (The ring is deeper than the requests a caller can
// have in flight between two synchronisations: one per temperature.)
// (REF_STATUS_CELL0, REF_STATUS_CELLS: asmc_scratch.h)
static int ref_status_request(asmc_ctx* ctx, const double* d_status, hipStream_t st) {
    ctx->ref_status_gen++;
    double* cell = ctx->h_pinned + REF_STATUS_CELL0 + ctx->ref_status_gen % REF_STATUS_CELLS;
    *cell = -2.0;
    ASMC_HIP(hipMemcpyAsync(cell, d_status, sizeof(double), hipMemcpyDeviceToHost, st));
    return ASMC_OK;
}

int asmc_ref_factor_launch(asmc_ctx* ctx, int d, const double* sum, const double* gram, double n_mean, double denom, double* out,
                           double* status, double* tab, double* em, int it, hipStream_t st) {
    const size_t lds = sizeof(double) * (size_t)d * (d + 1);
    static size_t attr_lds_dev[ASMC_MAX_DEVICES] = {0}; size_t& attr_lds = attr_lds_dev[asmc_dev_slot(ctx)];
    if (lds > 64 * 1024 && lds > attr_lds) {
        ASMC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ref_factor), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_lds = lds;
    }
    // d <= 32 is bound by the per-column latency whatever the block (38-41 us from 256 to 1024 threads); d = 128 by the trailing
    // updates: 683 us with 256 threads, 516 with 1024
    // (ASMC_REF_THREADS is a debugging knob for that measurement: a block smaller than d threads is not supported by the kernel -
    // its last passes give every column a thread - and no test covers the knob)
    static const int ref_env = getenv("ASMC_REF_THREADS") ? atoi(getenv("ASMC_REF_THREADS")) : 0;
    const int ref_threads = ref_env > 0 ? ref_env : (d <= 32 ? REF_THREADS : 1024);
    ASMC_LAUNCH(ctx, st, "k_ref_factor", k_ref_factor, dim3(1), dim3(ref_threads), lds, st, d, sum, gram, n_mean, denom, out,
                status, tab, em, it);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}
extern "C" {

// (mu, L, Linv) of the reference Gaussian from the moments of the pending asmc_mean_gram_enqueue (consumed: no fetch
// follows) or, with sum_host / gram_host, from moments the caller merged on the host (uploaded first): k_ref_factor on the
// stream.  The status lands in pinned memory behind it; asmc_reference_factor_status reads it after the caller's next
// synchronisation of the stream.
int asmc_reference_factor(asmc_ctx* ctx, int d, int64_t n_mean, int64_t n_cov, const double* sum_host, const double* gram_host,
                          double* out_dev, asmc_stream stream) {
    ASMC_REQUIRE(ctx && out_dev, "null pointer");
    ASMC_REQUIRE(d > 0 && d <= 128 && n_mean > 0 && n_cov > 0, "bad sizes (d <= 128)");
    ASMC_REQUIRE((sum_host == nullptr) == (gram_host == nullptr), "sum_host and gram_host come together");
    hipStream_t st = as_stream(stream);
    if (gram_host) {
        ASMC_REQUIRE(ctx->gram_pending_d == 0, "an asmc_mean_gram_enqueue is pending: its results would be overwritten");
        ASMC_HIP(hipStreamSynchronize(st));  // (the pinned staging may still feed an earlier copy)
        memcpy(ctx->h_gram, sum_host, sizeof(double) * d);
        memcpy(ctx->h_gram + 128, gram_host, sizeof(double) * d * d);
        ASMC_HIP(hipMemcpyAsync(ctx->d_ref, ctx->h_gram, sizeof(double) * (128 + (size_t)d * d), hipMemcpyHostToDevice, st));
    } else {
        ASMC_REQUIRE(ctx->gram_pending_d == d, "no asmc_mean_gram_enqueue of this d is pending");
        ctx->gram_pending_d = 0;
    }
    double* d_status = ctx->d_small + DS_REF_STATUS;
    const int rc = asmc_ref_factor_launch(ctx, d, ctx->d_ref, ctx->d_ref + 128, (double)n_mean, (double)(n_cov - 1 > 1 ? n_cov - 1 : 1),
                                          out_dev, d_status, nullptr, nullptr, 0, st);
    if (rc) return rc;
    return ref_status_request(ctx, d_status, st);
}

// The sharded form of the same fit without a host round trip: column sums and the centred Gram matrix into the CALLER's device
// buffers (the caller sums each over the ranks with its own stream-ordered all-reduce), then the factorisation from them.
__global__ __launch_bounds__(256) void k_copy_doubles(int n, const double* __restrict__ src, double* __restrict__ dst) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < n) dst[e] = src[e];
}

int asmc_colsum_dev(asmc_ctx* ctx, int64_t n, int d, int x_dtype, const void* x, int from_gather_flag, double* sum_dev,
                    asmc_stream stream) {
    ASMC_REQUIRE(ctx && x && sum_dev, "null pointer");
    ASMC_REQUIRE(n > 0 && d > 0 && d <= ctx->d_max && d <= ASMC_BLOCK, "bad sizes");
    ASMC_REQUIRE(x_dtype == ASMC_F64 || x_dtype == ASMC_F32, "bad x_dtype");
    hipStream_t st = as_stream(stream);
    int grid = grid_for(n, (ASMC_BLOCK / d) * 16, ctx->gram_blocks);
    const bool from_gather = from_gather_flag && ctx->cs_n == n && ctx->cs_x == x && ctx->cs_d == d && x_dtype == ASMC_F64;  // (see asmc_mean_gram_enqueue)
    if (from_gather)
        grid = ctx->cs_grid;
    else if (x_dtype == ASMC_F64)
        ASMC_LAUNCH(ctx, st, "k_colsum<double>", k_colsum<double>, dim3(grid), dim3(ASMC_BLOCK), ASMC_BLOCK * sizeof(double), st, n, d, (const double*)x, ctx->d_gram);
    else
        ASMC_LAUNCH(ctx, st, "k_colsum<float>", k_colsum<float>, dim3(grid), dim3(ASMC_BLOCK), ASMC_BLOCK * sizeof(double), st, n, d, (const float*)x, ctx->d_gram);
    ASMC_LAUNCH_CHECK();
    ASMC_LAUNCH(ctx, st, "k_reduce_columns", k_reduce_columns, dim3(d), dim3(from_gather ? 256 : 64), 0, st, grid, d, (const double*)ctx->d_gram, sum_dev);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int asmc_centered_gram_dev(asmc_ctx* ctx, int64_t n, int d, int x_dtype, const void* x, const double* sum_dev, int64_t n_mean,
                           double* gram_dev, asmc_stream stream) {
    ASMC_REQUIRE(ctx && x && sum_dev && gram_dev, "null pointer");
    ASMC_REQUIRE(n > 0 && n_mean > 0 && d > 0 && d <= ctx->d_max && d <= 128, "bad sizes (gram supports d <= 128)");
    ASMC_REQUIRE(x_dtype == ASMC_F64 || x_dtype == ASMC_F32, "bad x_dtype");
    if (!asmc_gram_mm_supported(d, x) || getenv("ASMC_GRAM_GENERIC")) {
        asmc_set_error("asmc_centered_gram_dev: shape without the matrix-core Gram kernel (d in {32, 64, 128}, 16-byte aligned rows)");
        return ASMC_ERR_UNSUPPORTED;
    }
    hipStream_t st = as_stream(stream);
    double* d_center = ctx->d_small + DS_GRAM_CENTER;
    ASMC_LAUNCH(ctx, st, "k_center_from_sum", k_center_from_sum, dim3(1), dim3(128), 0, st, d, sum_dev, (double)n_mean, d_center);
    ASMC_LAUNCH_CHECK();
    int ggrid = 0;
    const int rc = asmc_gram_mm_launch(ctx, n, d, x_dtype, x, d_center, &ggrid, st, nullptr, 0.0);
    if (rc) return rc;
    ASMC_LAUNCH(ctx, st, "k_copy_doubles", k_copy_doubles, dim3((d * d + 255) / 256), dim3(256), 0, st, d * d, (const double*)ctx->d_partials,
                gram_dev);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

int asmc_reference_factor_dev(asmc_ctx* ctx, int d, int64_t n_mean, int64_t n_cov, const double* sum_dev, const double* gram_dev,
                              double* out_dev, asmc_stream stream) {
    ASMC_REQUIRE(ctx && sum_dev && gram_dev && out_dev, "null pointer");
    ASMC_REQUIRE(d > 0 && d <= 128 && n_mean > 0 && n_cov > 0, "bad sizes (d <= 128)");
    hipStream_t st = as_stream(stream);
    double* d_status = ctx->d_small + DS_REF_STATUS;
    const int rc = asmc_ref_factor_launch(ctx, d, sum_dev, gram_dev, (double)n_mean, (double)(n_cov - 1 > 1 ? n_cov - 1 : 1), out_dev,
                                          d_status, nullptr, nullptr, 0, st);
    if (rc) return rc;
    return ref_status_request(ctx, d_status, st);
}

int asmc_reference_factor_status(asmc_ctx* ctx, int* status_host) {
    ASMC_REQUIRE(ctx && status_host, "null pointer");
    *status_host = (int)ctx->h_pinned[REF_STATUS_CELL0 + ctx->ref_status_gen % REF_STATUS_CELLS];  // -2: the stream has not been synchronised since asmc_reference_factor
    return ASMC_OK;
}

// the request a caller has just made, and the status of one particular request: a mutation asks about the factorisation
// that served IT - the next temperature's may already be on the stream behind it (asmc_reference_factor_status reads the latest
// request's cell: -2 until that one has run)
int64_t asmc_reference_factor_generation(asmc_ctx* ctx) { return ctx ? (int64_t)ctx->ref_status_gen : -1; }
int asmc_reference_factor_status_of(asmc_ctx* ctx, int64_t generation, int* status_host) {
    ASMC_REQUIRE(ctx && status_host, "null pointer");
    ASMC_REQUIRE(generation > 0 && (uint64_t)generation <= ctx->ref_status_gen &&
                     ctx->ref_status_gen - (uint64_t)generation < REF_STATUS_CELLS,
                 "no such factorisation request (or more than 15 requests ago)");
    *status_host = (int)ctx->h_pinned[REF_STATUS_CELL0 + (unsigned)generation % REF_STATUS_CELLS];
    return ASMC_OK;
}

int asmc_mean_gram(asmc_ctx* ctx, int64_t n, int d, int x_dtype, const void* x, int64_t n_mean, int across_ranks,
                   double* sum_host, double* gram_host, asmc_stream stream) {
    ASMC_REQUIRE(ctx && x && sum_host && gram_host, "null pointer");
    ASMC_REQUIRE(n > 0 && n_mean > 0 && d > 0 && d <= ctx->d_max && d <= 128, "bad sizes (gram supports d <= 128)");
    if (!across_ranks && (!(asmc_gram_mm_supported(d, x) && d <= ASMC_BLOCK) || getenv("ASMC_GRAM_GENERIC"))) {
        int rc = asmc_colsum(ctx, n, d, x_dtype, x, sum_host, stream);  // shapes without the fp64-MFMA Gram kernel
        if (rc) return rc;
        double center[128];
        for (int j = 0; j < d; j++) center[j] = sum_host[j] / (double)n_mean;
        return asmc_centered_gram(ctx, n, d, x_dtype, x, center, gram_host, stream);
    }
    const int rc = asmc_mean_gram_enqueue(ctx, n, d, x_dtype, x, n_mean, across_ranks, stream);
    if (rc) return rc;
    return asmc_mean_gram_fetch(ctx, d, sum_host, gram_host, stream);
}

int asmc_centered_gram(asmc_ctx* ctx, int64_t n, int d, int x_dtype, const void* x, const double* center_host,
                       double* gram_host, asmc_stream stream) {
    ASMC_REQUIRE(ctx && x && center_host && gram_host, "null pointer");
    ASMC_REQUIRE(n > 0 && d > 0 && d <= ctx->d_max && d <= 128, "bad sizes (gram supports d <= 128)");
    ASMC_REQUIRE(x_dtype == ASMC_F64 || x_dtype == ASMC_F32, "bad x_dtype");
    hipStream_t st = as_stream(stream);
    ASMC_HIP(hipStreamSynchronize(st));
    memcpy(ctx->h_pinned + HP_GRAM_CENTER, center_host, sizeof(double) * d);
    double* d_center = ctx->d_small + DS_GRAM_CENTER;
    ASMC_HIP(hipMemcpyAsync(d_center, ctx->h_pinned + HP_GRAM_CENTER, sizeof(double) * d, hipMemcpyHostToDevice, st));
    const size_t elem = x_dtype == ASMC_F64 ? 8 : 4;
    const int rowbytes = (int)(d * elem);
    double* d_out = ctx->d_partials;
    if (asmc_gram_mm_supported(d, x) && ctx->d_max >= d && !getenv("ASMC_GRAM_GENERIC")) {  // fp64 MFMA (asmc_pcn_mm.hip)
        int grid = 0;
        int rc = asmc_gram_mm_launch(ctx, n, d, x_dtype, x, d_center, &grid, st, nullptr, 0.0);
        if (rc) return rc;
        ASMC_HIP(hipMemcpyAsync(gram_host, d_out, sizeof(double) * d * d, hipMemcpyDeviceToHost, st));
        ASMC_HIP(hipStreamSynchronize(st));
        return ASMC_OK;
    }
    {
        // any other d <= 128: a zero-padded copy of the rows (centre padded with zeros) through the matrix-core kernel of the next
        // width >= 32; the d x d corner of its result is the answer (k_gram_rb took 1 ms at d = 48 and 8.5 ms at d = 100 per call)
        const int D = pcn_pad_dim(d) < 32 ? 32 : pcn_pad_dim(d);
        if (D > 0 && D != d && D <= (ctx->d_max_pad < 32 ? 32 : ctx->d_max_pad) && !getenv("ASMC_GRAM_GENERIC") && !pcn_env_nopad()) {
            int rc = pcn_xpad_reserve(ctx, (size_t)n * D * elem, st, "centered_gram: no device memory for the zero-padded copy of the rows");
            if (rc) return rc;
            for (int j = d; j < D; j++) ctx->h_pinned[HP_GRAM_CENTER + j] = 0.0;
            ASMC_HIP(hipMemcpyAsync(d_center, ctx->h_pinned + HP_GRAM_CENTER, sizeof(double) * D, hipMemcpyHostToDevice, st));
            rc = launch_pad_rows(ctx, n, d, D, x_dtype, x, ctx->d_xpad, st);
            if (rc) return rc;
            int grid = 0;
            rc = asmc_gram_mm_launch(ctx, n, D, x_dtype, ctx->d_xpad, d_center, &grid, st, nullptr, 0.0);
            if (rc) return rc;
            ASMC_HIP(hipMemcpy2DAsync(gram_host, sizeof(double) * d, d_out, sizeof(double) * D, sizeof(double) * d, d,
                                      hipMemcpyDeviceToHost, st));
            ASMC_HIP(hipStreamSynchronize(st));
            return ASMC_OK;
        }
    }
    if (rowbytes % 16 == 0 && ((uintptr_t)x % 16) == 0 && d <= 128) {
        // register-blocked kernel: BLK = 4 (quadrant 32) for d <= 32, else BLK = 8 (quadrant 64)
        const int blk = d <= 32 ? 4 : 8;
        const int Q = 8 * blk;
        const int nq = (d + Q - 1) / Q;
        const int dpad = nq * Q;
        const int wpb = d > 64 ? 2 : ASMC_BLOCK / 64;  // d = 128: two waves per block keep the tiles inside 160 KB of LDS
        const size_t lds = (size_t)wpb * 64 * lds_row_stride(rowbytes);
        const size_t lds_red = (size_t)wpb * Q * Q * sizeof(double);
        const size_t lds_bytes = lds > lds_red ? lds : lds_red;
        int cap = (int)(((size_t)ctx->gram_blocks * ctx->d_max * ctx->d_max) / ((size_t)dpad * dpad));
        if (cap > ctx->num_cu * 2) cap = ctx->num_cu * 2;
        if (cap < 1) {
            asmc_set_error("centered_gram: ctx d_max=%d too small for d=%d", ctx->d_max, d);
            return ASMC_ERR_ARG;
        }
        const int grid = grid_for((n + 63) / 64, wpb, cap);
        auto launch = [&](auto kern, auto xp) {
            if (lds_bytes > 64 * 1024)
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
            ASMC_LAUNCH(ctx, st, "k_gram_rb", kern, dim3(grid, nq * nq), dim3(wpb * 64), lds_bytes, st, n, d, xp,
                        (const double*)d_center, ctx->d_gram, nq);
        };
        if (x_dtype == ASMC_F64) {
            if (blk == 4) launch(k_gram_rb<double, 4>, (const double*)x);
            else launch(k_gram_rb<double, 8>, (const double*)x);
        } else {
            if (blk == 4) launch(k_gram_rb<float, 4>, (const float*)x);
            else launch(k_gram_rb<float, 8>, (const float*)x);
        }
        ASMC_LAUNCH_CHECK();
        ASMC_LAUNCH(ctx, st, "k_reduce_columns", k_reduce_columns, dim3(dpad * dpad < 1024 ? dpad * dpad : 1024), dim3(64), 0, st, grid,
                    dpad * dpad, (const double*)ctx->d_gram, d_out);
        ASMC_LAUNCH_CHECK();
        // strip the padding while copying back
        ASMC_HIP(hipMemcpy2DAsync(gram_host, sizeof(double) * d, d_out, sizeof(double) * dpad, sizeof(double) * d, d,
                                  hipMemcpyDeviceToHost, st));
        ASMC_HIP(hipStreamSynchronize(st));
        return ASMC_OK;
    }
    ASMC_REQUIRE(d <= 64, "centered_gram: unaligned rows are supported for d <= 64 only");
    const int grid = grid_for(n, 64 * 8, ctx->gram_blocks);
    const size_t lds = sizeof(double) * 64 * (d + 1);
    if (x_dtype == ASMC_F64)
        ASMC_LAUNCH(ctx, st, "k_gram<double>", k_gram<double>, dim3(grid), dim3(ASMC_BLOCK), lds, st, n, d, (const double*)x, (const double*)d_center, ctx->d_gram);
    else
        ASMC_LAUNCH(ctx, st, "k_gram<float>", k_gram<float>, dim3(grid), dim3(ASMC_BLOCK), lds, st, n, d, (const float*)x, (const double*)d_center, ctx->d_gram);
    ASMC_LAUNCH_CHECK();
    // d*d <= 4096 doubles: reduce into d_partials, then read back
    ASMC_LAUNCH(ctx, st, "k_reduce_columns", k_reduce_columns, dim3(d * d < 1024 ? d * d : 1024), dim3(64), 0, st, grid, d * d, (const double*)ctx->d_gram, d_out);
    ASMC_LAUNCH_CHECK();
    ASMC_HIP(hipMemcpyAsync(gram_host, d_out, sizeof(double) * d * d, hipMemcpyDeviceToHost, st));
    ASMC_HIP(hipStreamSynchronize(st));
    return ASMC_OK;
}

}  // extern "C"
