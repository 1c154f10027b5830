// asmc_nsf.hip — neural spline flow (include/asmc.h ASMC_FLOW_NSF): packing, density and draw on the CDNA4 matrix cores.
//
// Reference: examples/smc_example.py:82 asks zuko for flow_class="NSF" (ZukoFlow forwards any class name,
// src/aspire/flows/torch/flows.py:155-164); its density is evaluated n_steps times per temperature in the mutation loop
// (samplers/smc/base.py:507-519 around flows.py:368-387) and its draw once per run (flows.py:327-346).  zuko is absent: the flow
// is this repository's NSFFlow (aspire_amd/flows.py) - standardise, then n_layers masked autoregressive transforms whose MADE
// network  d -> W -> W -> d (3 K - 1)  (ReLU) emits the K = 8 widths, 8 heights and 7 interior derivatives of a monotonic
// rational-quadratic spline per coordinate (asmc_nsf_dev.h);  log q(x) = N(z; 0, I) + sum log J - sum log scale.
//
// Mapping.  16-particle groups on v_mfma_f32_16x16x32_f16, four lanes per particle (asmc_flow16_dev.h: split-fp16 products, the
// accumulators of one layer are the B operand of the next).  Lane (p = l & 15, g = l >> 4) holds the coordinates
//     coordinate(cg, g, r) = 16 cg + 4 g + r,   r = 0 .. 3,  cg = 0 .. NCG - 1   (NCG = 1 for d <= 16, 2 for d <= 32)
// of particle p.  The output layer's rows are packed PARAMETER-major per group of 16 coordinates: output block (cg, c) holds
// parameter c of the coordinates 16 cg .. 16 cg + 15, so that accumulator register r of lane (p, g) is parameter c of the lane's
// own coordinate (cg, g, r) - softmax, cumulative knots, bin search and the rational-quadratic map are lane local, and no
// parameter ever leaves the registers.  A particle never holds more than the 8 parameters x 4 coordinates of one chunk:
// the 8 width blocks are reduced to (bin, left knot, width), the 8 height blocks to (left knot, height) of that bin, the 7
// derivative blocks to the bin's two knot derivatives.
//
// Weights are streamed (the output layer of ONE transform is 184 KB of (hi, lo) halves at d = 32, W = 64): per transform the
// chunks  [A1 | A2]  and, per coordinate group,  [8 width blocks] [8 height blocks] [7 derivative blocks]  go through two LDS
// slots by global_load_lds, chunk q + 1 in flight while the block computes on chunk q, one workgroup barrier per chunk.  A weight
// word is used once per particle, so a chunk has to serve many particles: every wave carries G 16-particle groups through a
// chunk, their hidden activations kept as packed (hi, lo) operands in registers - 8 waves x G x 16 particles per chunk.
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "asmc_common.h"
#include "asmc_pcn_dev.h"  // normal_quad_f32
#include "asmc_flow16_dev.h"
#include "asmc_nsf_dev.h"

#define NSF_THREADS 512
#define NSF_G_LOGPROB 2  // 16-particle groups per wave and chunk: 256 particles per workgroup and chunk
#define NSF_G_SAMPLE 1

template <int W>
struct Nsf {
    static_assert(W == 32 || W == 64, "hidden width");
    static constexpr int KS2 = W / 32;           // K = 32 steps of a layer that reads a hidden layer (the first layer: one step)
    static constexpr int NB1 = W / 16;           // 16-row output blocks of a hidden layer
    static constexpr int BLK1 = 512, BLK2 = KS2 * 512;  // words per output block: (hi, lo) images of every K step
    static constexpr int A1 = NB1 * BLK1, A2 = NB1 * BLK2, HEAD = A1 + A2;
    static constexpr int CW = NSF_BINS * BLK2;   // words per LDS slot: eight output blocks
    static_assert(HEAD <= CW, "the two hidden layers are one chunk");
    static constexpr __host__ __device__ int nb3(int ncg) { return ncg * NSF_PARAMS; }
    static constexpr __host__ __device__ int layer_a(int ncg) { return HEAD + nb3(ncg) * BLK2; }
    static constexpr __host__ __device__ int bias(int ncg) { return 2 * W + nb3(ncg) * 16; }
    static constexpr __host__ __device__ int nchunks(int ncg) { return 1 + 3 * ncg; }
    // chunk c of a transform: 0 = [A1 | A2]; 1 + 3 cg + {0, 1, 2} = widths / heights / derivatives of coordinate group cg
    static constexpr __host__ __device__ int first_block(int c) { return ((c - 1) / 3) * NSF_PARAMS + ((c - 1) % 3) * NSF_BINS; }
    static constexpr __host__ __device__ int chunk_off(int c) { return c == 0 ? 0 : HEAD + first_block(c) * BLK2; }
    static constexpr __host__ __device__ int chunk_words(int c) { return c == 0 ? HEAD : ((c - 1) % 3 == 2 ? NSF_BINS - 1 : NSF_BINS) * BLK2; }
};

static int nsf_ncg(int dims) { return dims <= 16 ? 1 : 2; }
static bool nsf_supported(int dims, int hidden, int bins) { return dims >= 1 && dims <= 32 && (hidden == 32 || hidden == 64) && bins == NSF_BINS; }

// The weight stream: two LDS slots of FD::CW words; the caller names the chunk that goes into flight behind the current one.
template <class FD, int THREADS>
struct NsfStream {
    const float* __restrict__ gA;
    float* slots;
    int ncg;
    unsigned parity;  // slot of the chunk that is IN FLIGHT

    __device__ __forceinline__ void issue(int t, int c, unsigned slot) {
        const int off = t * FD::layer_a(ncg) + FD::chunk_off(c);
        const int words = FD::chunk_words(c);
        constexpr int WAVES = THREADS / 64;
        // (the wave index as a scalar: asmc_flow16_dev.h Flow16Stream::issue)
        const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
        for (int q = wave; q * 256 < words; q += WAVES) {
            const float* src = gA + off + q * 256 + lane * 4;
            float* dst = slots + slot * FD::CW + q * 256;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
        }
    }
    __device__ __forceinline__ void start(const float* g, float* s, int ncg_, int t0) {
        gA = g, slots = s, ncg = ncg_, parity = 0;
        issue(t0, 0, 0);
    }
    // the chunk in flight has landed and every wave is past the one before it; chunk (nt, nc) goes into flight
    __device__ __forceinline__ const float* next(int nt, int nc) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const float* cur = slots + parity * FD::CW;
        parity ^= 1u;
        issue(nt, nc, parity);
        return cur;
    }
    // the chunk in flight is not the one needed next (block-uniform decision): chunk 0 of transform t in its place
    __device__ __forceinline__ void redirect(int t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        issue(t, 0, parity);
    }
};

// The two hidden layers of one transform for the wave's G groups: xs[j] = the lane's coordinates of group j (slot s = 4 cg + r),
// (bh, bl)[j] = relu(hidden 2) as the output layer's B operand.
template <class FD, int W, int NCG, int G>
__device__ __forceinline__ void nsf_hidden(const float (&xs)[G][4 * NCG], half8 (&bh)[G][FD::KS2], half8 (&bl)[G][FD::KS2], const float* __restrict__ A,
                                           const float* __restrict__ bias, int lane, unsigned (&amax)[G]) {
    constexpr int KS2 = FD::KS2, NB1 = FD::NB1;
#pragma unroll
    for (int j = 0; j < G; j++) {
        float v[8];
#pragma unroll
        for (int s = 0; s < 8; s++) v[s] = s < 4 * NCG ? xs[j][s < 4 * NCG ? s : 0] : 0.0f;  // K index 16 (s / 4) + 4 g + s % 4 = the coordinate
        half8 xh[1], xl[1];
        f16_split8<false>(v, xh[0], xl[0], amax[j]);
        floatx4 h1[NB1];
        f16_dense<NB1, 1>(h1, xh, xl, A, bias, lane);
        half8 ch[KS2], cl[KS2];
#pragma unroll
        for (int S = 0; S < KS2; S++) {
#pragma unroll
            for (int s = 0; s < 8; s++) v[s] = h1[2 * S + s / 4][s % 4];
            f16_split8<true>(v, ch[S], cl[S], amax[j]);
        }
        floatx4 h2[NB1];
        f16_dense<NB1, KS2>(h2, ch, cl, A + FD::A1, bias + W, lane);
#pragma unroll
        for (int S = 0; S < KS2; S++) {
#pragma unroll
            for (int s = 0; s < 8; s++) v[s] = h2[2 * S + s / 4][s % 4];
            f16_split8<true>(v, bh[j][S], bl[j][S], amax[j]);
        }
        __builtin_amdgcn_sched_barrier(0);  // one group's chain at a time: interleaved, the G chains' accumulators do not fit the registers
    }
}

// One transform, data -> latent, of the wave's G groups (in place; every conditioner input is converted before a coordinate
// changes).  `t`: the transform, `t_next`: the one whose first chunk goes into flight behind this one's last.
template <class FD, int W, int NCG, int G>
__device__ __forceinline__ void nsf_transform(float (&xs)[G][4 * NCG], const float* __restrict__ bias, NsfStream<FD, NSF_THREADS>& stream, int t,
                                              int t_next, int lane, float (&ladj)[G], unsigned (&amax)[G]) {
    constexpr int KS2 = FD::KS2, NCH = FD::nchunks(NCG);
    half8 bh[G][KS2], bl[G][KS2];
    nsf_hidden<FD, W, NCG, G>(xs, bh, bl, stream.next(t, 1), bias, lane, amax);
    const float* ob = bias + 2 * W;
    // (one instance per coordinate group, the group a compile-time constant: as a loop the body is past the unroller's budget and
    // the lane's coordinate arrays, indexed by a variable, would leave the registers)
    auto group = [&](auto cgc) __attribute__((always_inline)) {
        constexpr int cg = decltype(cgc)::value;
        int kk[G][4];
        float x0[G][4], wd[G][4], y0[G][4], ht[G][4];
        {
            const float* A = stream.next(t, 3 * cg + 2);
#pragma unroll
            for (int j = 0; j < G; j++) {
                floatx4 o[NSF_BINS];
                __builtin_amdgcn_sched_barrier(0);
                f16_dense<NSF_BINS, KS2>(o, bh[j], bl[j], A, ob + (cg * NSF_PARAMS) * 16, lane);
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    float raw[NSF_BINS], kn[NSF_BINS - 1], hi;
#pragma unroll
                    for (int c = 0; c < NSF_BINS; c++) raw[c] = o[c][r];
                    nsf_knots(raw, kn);
                    nsf_locate(kn, xs[j][4 * cg + r], kk[j][r], x0[j][r], hi);
                    wd[j][r] = hi - x0[j][r];
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        {
            const float* A = stream.next(t, 3 * cg + 3);
#pragma unroll
            for (int j = 0; j < G; j++) {
                floatx4 o[NSF_BINS];
                __builtin_amdgcn_sched_barrier(0);
                f16_dense<NSF_BINS, KS2>(o, bh[j], bl[j], A, ob + (cg * NSF_PARAMS + NSF_BINS) * 16, lane);
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    float raw[NSF_BINS], kn[NSF_BINS - 1], hi;
#pragma unroll
                    for (int c = 0; c < NSF_BINS; c++) raw[c] = o[c][r];
                    nsf_knots(raw, kn);
                    asm volatile("" : "+v"(kk[j][r]));  // (opaque: the compiler otherwise keeps the eight lane masks k == c of every coordinate alive from one chunk to the next)
                    nsf_bin_knots(kn, kk[j][r], y0[j][r], hi);
                    ht[j][r] = hi - y0[j][r];
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        {
            const bool last = 3 * cg + 4 == NCH;
            const float* A = stream.next(last ? t_next : t, last ? 0 : 3 * cg + 4);
#pragma unroll
            for (int j = 0; j < G; j++) {
                floatx4 o[NSF_BINS - 1];
                __builtin_amdgcn_sched_barrier(0);
                f16_dense<NSF_BINS - 1, KS2>(o, bh[j], bl[j], A, ob + (cg * NSF_PARAMS + 2 * NSF_BINS) * 16, lane);
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    float raw[NSF_BINS - 1], d0, d1, y, lj;
#pragma unroll
                    for (int c = 0; c < NSF_BINS - 1; c++) raw[c] = o[c][r];
                    asm volatile("" : "+v"(kk[j][r]));  // (opaque: the compiler otherwise keeps the eight lane masks k == c of every coordinate alive from one chunk to the next)
                    nsf_bin_derivs(raw, kk[j][r], d0, d1);
                    nsf_forward(xs[j][4 * cg + r], kk[j][r], x0[j][r], wd[j][r], y0[j][r], ht[j][r], d0, d1, y, lj);
                    xs[j][4 * cg + r] = y;
                    ladj[j] += lj;
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    };
    group(std::integral_constant<int, 0>{});
    if constexpr (NCG > 1) group(std::integral_constant<int, 1>{});
}

// One pass of the inversion of a transform: xn = spline^-1(z; theta(xc)) on all coordinates, lj = sum log J (data -> latent) at xn.
// `t_spec`: the transform whose first chunk goes into flight behind this pass's last (the same transform again, unless the
// caller knows this pass to be the last).
template <class FD, int W, int NCG, int G>
__device__ __forceinline__ void nsf_inverse_pass(const float (&xc)[G][4 * NCG], const float (&zs)[G][4 * NCG], float (&xn)[G][4 * NCG],
                                                 const float* __restrict__ bias, NsfStream<FD, NSF_THREADS>& stream, int t, int t_spec, int lane,
                                                 float (&lj_pass)[G], unsigned (&amax)[G]) {
    constexpr int KS2 = FD::KS2, NCH = FD::nchunks(NCG);
    half8 bh[G][KS2], bl[G][KS2];
    nsf_hidden<FD, W, NCG, G>(xc, bh, bl, stream.next(t, 1), bias, lane, amax);
    const float* ob = bias + 2 * W;
    // (one instance per coordinate group, the group a compile-time constant: as a loop the body is past the unroller's budget and
    // the lane's coordinate arrays, indexed by a variable, would leave the registers)
    auto group = [&](auto cgc) __attribute__((always_inline)) {
        constexpr int cg = decltype(cgc)::value;
        float xk[G][4][NSF_BINS - 1];
        int kk[G][4];
        float x0[G][4], wd[G][4], y0[G][4], ht[G][4];
        {
            const float* A = stream.next(t, 3 * cg + 2);
#pragma unroll
            for (int j = 0; j < G; j++) {
                floatx4 o[NSF_BINS];
                __builtin_amdgcn_sched_barrier(0);
                f16_dense<NSF_BINS, KS2>(o, bh[j], bl[j], A, ob + (cg * NSF_PARAMS) * 16, lane);
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    float raw[NSF_BINS];
#pragma unroll
                    for (int c = 0; c < NSF_BINS; c++) raw[c] = o[c][r];
                    nsf_knots(raw, xk[j][r]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        {
            const float* A = stream.next(t, 3 * cg + 3);
#pragma unroll
            for (int j = 0; j < G; j++) {
                floatx4 o[NSF_BINS];
                __builtin_amdgcn_sched_barrier(0);
                f16_dense<NSF_BINS, KS2>(o, bh[j], bl[j], A, ob + (cg * NSF_PARAMS + NSF_BINS) * 16, lane);
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    float raw[NSF_BINS], kn[NSF_BINS - 1], hi;
#pragma unroll
                    for (int c = 0; c < NSF_BINS; c++) raw[c] = o[c][r];
                    nsf_knots(raw, kn);
                    nsf_locate(kn, zs[j][4 * cg + r], kk[j][r], y0[j][r], hi);  // the bin is found on Y
                    ht[j][r] = hi - y0[j][r];
                    nsf_bin_knots(xk[j][r], kk[j][r], x0[j][r], hi);
                    wd[j][r] = hi - x0[j][r];
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        {
            const bool last = 3 * cg + 4 == NCH;
            const float* A = stream.next(last ? t_spec : t, last ? 0 : 3 * cg + 4);
#pragma unroll
            for (int j = 0; j < G; j++) {
                floatx4 o[NSF_BINS - 1];
                __builtin_amdgcn_sched_barrier(0);
                f16_dense<NSF_BINS - 1, KS2>(o, bh[j], bl[j], A, ob + (cg * NSF_PARAMS + 2 * NSF_BINS) * 16, lane);
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    float raw[NSF_BINS - 1], d0, d1, lj;
#pragma unroll
                    for (int c = 0; c < NSF_BINS - 1; c++) raw[c] = o[c][r];
                    asm volatile("" : "+v"(kk[j][r]));  // (opaque: the compiler otherwise keeps the eight lane masks k == c of every coordinate alive from one chunk to the next)
                    nsf_bin_derivs(raw, kk[j][r], d0, d1);
                    nsf_inverse(zs[j][4 * cg + r], kk[j][r], x0[j][r], wd[j][r], y0[j][r], ht[j][r], d0, d1, xn[j][4 * cg + r], lj);
                    lj_pass[j] += lj;
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    };
    group(std::integral_constant<int, 0>{});
    if constexpr (NCG > 1) group(std::integral_constant<int, 1>{});
}

// LDS: [2 x CW weight slots][n_layers x bias][loc | scale | 1 / scale, 32 each, in coordinate order]
template <class FD, int NCG>
__device__ __forceinline__ void nsf_stage_tables(float* s_bias, float* s_loc, const float* __restrict__ packed, int n_layers, int d,
                                                 const float* __restrict__ loc, const float* __restrict__ scale) {
    for (int e = threadIdx.x; e < n_layers * FD::bias(NCG); e += NSF_THREADS) s_bias[e] = packed[e];
    for (int e = threadIdx.x; e < 32; e += NSF_THREADS) {
        s_loc[e] = e < d ? loc[e] : 0.0f;
        s_loc[32 + e] = e < d ? scale[e] : 1.0f;
        s_loc[64 + e] = e < d ? 1.0f / scale[e] : 1.0f;
    }
}

// log q of one group from its latent coordinates (every lane of a particle returns it)
template <int NCG>
__device__ __forceinline__ float nsf_finish(const float (&z)[4 * NCG], float ladj, unsigned amax_pk, float ladj0, float base_const) {
    float q = 0.0f;
#pragma unroll
    for (int s = 0; s < 4 * NCG; s++) q = fmaf(z[s], z[s], q);
    q = f16_quad_sum(q);
    const float lj = f16_quad_sum(ladj);
    float am = range_pk_max(amax_pk);
    am = (am != am) ? __builtin_inff() : am;
    am = f16_quad_max(am);
    // an operand past the fp16 range makes the split products garbage: NaN, never a finite wrong number
    return !(am < FLOW_HS_MAX) ? __builtin_nanf("") : (-0.5f * q + base_const) + (ladj0 + lj);
}

template <int W, int NCG, typename XT, int G>
__global__ __launch_bounds__(NSF_THREADS) void k_nsf_logprob(int64_t n, int d, const XT* __restrict__ x, const float* __restrict__ packed,
                                                            int n_layers, const float* __restrict__ loc, const float* __restrict__ scale,
                                                            float ladj0, float base_const, double* __restrict__ out) {
    using FD = Nsf<W>;
    extern __shared__ __align__(16) float sm[];
    constexpr int WAVES = NSF_THREADS / 64;
    float* slots = sm;
    float* s_bias = slots + 2 * FD::CW;
    float* s_loc = s_bias + n_layers * FD::bias(NCG);
    NsfStream<FD, NSF_THREADS> stream;
    stream.start(packed + (size_t)n_layers * FD::bias(NCG), slots, NCG, 0);
    nsf_stage_tables<FD, NCG>(s_bias, s_loc, packed, n_layers, d, loc, scale);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, p = lane & 15, g = lane >> 4;
    const int64_t n_groups = (n + 15) / 16;
    const int64_t per_round = (int64_t)gridDim.x * WAVES * G;
    const int64_t rounds = (n_groups + per_round - 1) / per_round;  // the same trip count for every wave: they share the stream's barriers
    for (int64_t it = 0; it < rounds; it++) {
        const int64_t grp0 = it * per_round + ((int64_t)blockIdx.x * WAVES + wave) * G;
        float xs[G][4 * NCG], ladj[G];
        unsigned amax[G];
#pragma unroll
        for (int j = 0; j < G; j++) {
            const int64_t row = (grp0 + j) * 16 + p;
            ladj[j] = 0.0f, amax[j] = 0u;
#pragma unroll
            for (int s = 0; s < 4 * NCG; s++) {
                const int c = 16 * (s / 4) + 4 * g + s % 4;  // padded coordinates stay at zero: zero weights give the identity spline on 0
                xs[j][s] = (row < n && c < d) ? flow_standardise((float)x[row * d + c], s_loc[c], s_loc[32 + c], s_loc[64 + c]) : 0.0f;
            }
        }
        for (int t = 0; t < n_layers; t++)  // (n_layers is uniform over the block: every wave meets the same barriers)
            nsf_transform<FD, W, NCG, G>(xs, s_bias + t * FD::bias(NCG), stream, t, t + 1 == n_layers ? 0 : t + 1, lane, ladj, amax);
#pragma unroll
        for (int j = 0; j < G; j++) {
            const int64_t row = (grp0 + j) * 16 + p;
            const float val = nsf_finish<NCG>(xs[j], ladj[j], amax[j], ladj0, base_const);
            if (row < n && g == 0) out[row] = (double)val;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the chunk the last next() put into flight
}

// Draw (flows/torch/flows.py:327-346): z ~ N(0, I) from the counter-based generator exactly as k_maf_sample draws it (coordinate c
// = element c % 4 of quad c / 4 of the particle's draw, keyed by seed, global particle index and draw_id), the transforms inverted
// in reverse order.  Inverting ONE transform iterates x <- spline^-1(z; theta(x)) on all coordinates from x = 0: after pass k every
// coordinate whose inputs have degree < k is final, so d passes fix them all; a pass that returns its input bit for bit - every
// coordinate of every particle of the BLOCK, whose waves share the weight stream's barriers - has found the fixed point and every
// further pass would return the same bits and the same log J, so the loop stops there with the d-pass result exactly.  The values of
// a spline are bounded by max(|z|, B): no clamp.  A NaN in any pass's output, or an operand past the fp16 range in any pass,
// makes the row's log q NaN.
template <int W, int NCG, typename XT, int G>
__global__ __launch_bounds__(NSF_THREADS) void k_nsf_sample(int64_t n, int d, const float* __restrict__ packed, int n_layers,
                                                           const float* __restrict__ loc, const float* __restrict__ scale, float ladj0,
                                                           float base_const, unsigned long long seed, unsigned long long gid0, uint32_t draw_id,
                                                           XT* __restrict__ x, double* __restrict__ out, int all_passes) {
    using FD = Nsf<W>;
    extern __shared__ __align__(16) float sm[];
    constexpr int WAVES = NSF_THREADS / 64;
    float* slots = sm;
    float* s_bias = slots + 2 * FD::CW;
    float* s_loc = s_bias + n_layers * FD::bias(NCG);
    NsfStream<FD, NSF_THREADS> stream;
    stream.start(packed + (size_t)n_layers * FD::bias(NCG), slots, NCG, n_layers - 1);
    nsf_stage_tables<FD, NCG>(s_bias, s_loc, packed, n_layers, d, loc, scale);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, p = lane & 15, g = lane >> 4;
    const int64_t n_groups = (n + 15) / 16;
    const int64_t per_round = (int64_t)gridDim.x * WAVES * G;
    const int64_t rounds = (n_groups + per_round - 1) / per_round;
    for (int64_t it = 0; it < rounds; it++) {
        const int64_t grp0 = it * per_round + ((int64_t)blockIdx.x * WAVES + wave) * G;
        float zs[G][4 * NCG], xs[G][4 * NCG], q[G], ladj[G];
        unsigned amax[G];
        bool bad[G];
#pragma unroll
        for (int j = 0; j < G; j++) {
            const int64_t row = (grp0 + j) * 16 + p;
            const unsigned long long gid = gid0 + (unsigned long long)(row < n ? row : n - 1);
            q[j] = 0.0f, ladj[j] = 0.0f, amax[j] = 0u, bad[j] = false;
#pragma unroll
            for (int cg = 0; cg < NCG; cg++) {
                double zq[4] = {0.0, 0.0, 0.0, 0.0};
                if (16 * cg + 4 * g < d) normal_quad_f32(seed, gid, draw_id, (uint32_t)(4 * cg + g), zq[0], zq[1], zq[2], zq[3]);
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    zs[j][4 * cg + r] = 16 * cg + 4 * g + r < d ? (float)zq[r] : 0.0f;
                    q[j] = fmaf(zs[j][4 * cg + r], zs[j][4 * cg + r], q[j]);
                }
            }
        }
        for (int t = n_layers - 1; t >= 0; t--) {
            const int t_after = t > 0 ? t - 1 : n_layers - 1;  // the transform that follows this one's last pass (the next round starts over)
#pragma unroll
            for (int j = 0; j < G; j++)
#pragma unroll
                for (int s = 0; s < 4 * NCG; s++) xs[j][s] = 0.0f;
            float lj_pass[G];
            for (int pass = 0; pass < d; pass++) {
                const bool final_pass = pass + 1 == d;
                float xn[G][4 * NCG];
#pragma unroll
                for (int j = 0; j < G; j++) lj_pass[j] = 0.0f;
                nsf_inverse_pass<FD, W, NCG, G>(xs, zs, xn, s_bias + t * FD::bias(NCG), stream, t, final_pass ? t_after : t, lane, lj_pass, amax);
                bool same = true;
#pragma unroll
                for (int j = 0; j < G; j++)
#pragma unroll
                    for (int s = 0; s < 4 * NCG; s++) {
                        same = same && (__float_as_uint(xn[j][s]) == __float_as_uint(xs[j][s]));
                        bad[j] = bad[j] || (xn[j][s] != xn[j][s]);  // every pass counts, not just the last
                        xs[j][s] = xn[j][s];
                    }
                if (final_pass) break;
                if (!all_passes && __syncthreads_and(same)) {  // (block uniform) the fixed point: this pass's log J was formed at final inputs
                    stream.redirect(t_after);
                    break;
                }
            }
#pragma unroll
            for (int j = 0; j < G; j++) {
                ladj[j] += lj_pass[j];
#pragma unroll
                for (int s = 0; s < 4 * NCG; s++) zs[j][s] = xs[j][s];
            }
        }
#pragma unroll
        for (int j = 0; j < G; j++) {
            const int64_t row = (grp0 + j) * 16 + p;
            // log q of the returned x: N(z) at the drawn latent plus the data -> latent log J of every transform's last pass
            float am = range_pk_max(amax[j]);
            am = (am != am || bad[j]) ? __builtin_inff() : am;
            am = f16_quad_max(am);
            const float qq = f16_quad_sum(q[j]);
            const float lj = f16_quad_sum(ladj[j]);
            const float val = !(am < FLOW_HS_MAX) ? __builtin_nanf("") : (-0.5f * qq + base_const) + (ladj0 + lj);
            if (row < n) {
#pragma unroll
                for (int s = 0; s < 4 * NCG; s++) {
                    const int c = 16 * (s / 4) + 4 * g + s % 4;
                    if (c < d) x[row * d + c] = (XT)(zs[j][s] * s_loc[32 + c] + s_loc[c]);
                }
                if (g == 0) out[row] = (double)val;
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---------------------------------------------------------------------------------------------------------------------------
// host side
static inline uint16_t nsf_f16_bits(_Float16 v) {
    uint16_t b;
    memcpy(&b, &v, 2);
    return b;
}

template <int W>
static int nsf_pack_w(int dims, int n_layers, const float* const* weights_host, const float* const* biases_host, float* packed_host) {
    using FD = Nsf<W>;
    const int ncg = nsf_ncg(dims), P = NSF_PARAMS;
    const int64_t sizes[3] = {(int64_t)W * dims, (int64_t)W * W, (int64_t)dims * P * W};
    for (int c = 0; c < 3 * n_layers; c++)
        for (int64_t k = 0; k < sizes[c % 3]; k++)
            if (!(fabsf(weights_host[c][k]) < 65504.0f)) {
                asmc_set_error("asmc_nsf_pack: weight %g of matrix %d is outside the fp16 operand range of the split-fp16 flow kernels (|w| < 65504)",
                               (double)weights_host[c][k], c);
                return ASMC_ERR_UNSUPPORTED;
            }
    float* bias = packed_host;
    uint16_t* img = reinterpret_cast<uint16_t*>(packed_host + (int64_t)n_layers * FD::bias(ncg));
    // [K step][hi | lo][lane][8 halves] inside an output block's image (asmc_flow16.hip pack16)
    auto put = [&](uint16_t* blockimg, int S, int lane, int j, float w) {
        const _Float16 hi = (_Float16)w;
        const _Float16 lo = (_Float16)(w - (float)hi);
        blockimg[((size_t)(S * 2 + 0) * 64 + lane) * 8 + j] = nsf_f16_bits(hi);
        blockimg[((size_t)(S * 2 + 1) * 64 + lane) * 8 + j] = nsf_f16_bits(lo);
    };
    // output block ob = cg * 23 + c, accumulator row m = 4 g + r: parameter c of coordinate 16 cg + m -> row of the torch output
    // layer (feature major: coordinate * 23 + c), or -1 for a padded coordinate
    auto out_row = [&](int ob, int m) {
        const int coord = 16 * (ob / P) + m;
        return coord < dims ? coord * P + ob % P : -1;
    };
    for (int t = 0; t < n_layers; t++) {
        const float *W1 = weights_host[3 * t], *W2 = weights_host[3 * t + 1], *W3 = weights_host[3 * t + 2];
        const float *B1 = biases_host[3 * t], *B2 = biases_host[3 * t + 1], *B3 = biases_host[3 * t + 2];
        float* b = bias + (int64_t)t * FD::bias(ncg);
        for (int u = 0; u < W; u++) b[u] = B1[u], b[W + u] = B2[u];
        for (int ob = 0; ob < FD::nb3(ncg); ob++)
            for (int m = 0; m < 16; m++) {
                const int o = out_row(ob, m);
                b[2 * W + ob * 16 + m] = o >= 0 ? B3[o] : 0.0f;
            }
        uint16_t* A1 = img + (size_t)t * FD::layer_a(ncg) * 2;
        uint16_t* A2 = A1 + (size_t)FD::A1 * 2;
        uint16_t* A3 = A2 + (size_t)FD::A2 * 2;
        for (int mbo = 0; mbo < FD::NB1; mbo++)
            for (int lane = 0; lane < 64; lane++)
                for (int j = 0; j < 8; j++) {
                    const int m = lane & 15, kg = lane >> 4;
                    const int in = 16 * (j / 4) + 4 * kg + j % 4;  // the coordinate held in slot j of lane group kg
                    put(A1 + (size_t)mbo * FD::BLK1 * 2, 0, lane, j, in < dims ? W1[(int64_t)(16 * mbo + m) * dims + in] : 0.0f);
                }
        for (int mbo = 0; mbo < FD::NB1; mbo++)
            for (int S = 0; S < FD::KS2; S++)
                for (int lane = 0; lane < 64; lane++)
                    for (int j = 0; j < 8; j++) {
                        const int m = lane & 15, kg = lane >> 4;
                        const int u = 16 * (2 * S + j / 4) + 4 * kg + j % 4;
                        put(A2 + (size_t)mbo * FD::BLK2 * 2, S, lane, j, W2[(int64_t)(16 * mbo + m) * W + u]);
                    }
        for (int ob = 0; ob < FD::nb3(ncg); ob++)
            for (int S = 0; S < FD::KS2; S++)
                for (int lane = 0; lane < 64; lane++)
                    for (int j = 0; j < 8; j++) {
                        const int m = lane & 15, kg = lane >> 4;
                        const int u = 16 * (2 * S + j / 4) + 4 * kg + j % 4;
                        const int o = out_row(ob, m);
                        put(A3 + (size_t)ob * FD::BLK2 * 2, S, lane, j, o >= 0 ? W3[(int64_t)o * W + u] : 0.0f);
                    }
    }
    return ASMC_OK;
}

extern "C" int64_t asmc_nsf_pack_floats(int dims, int n_transforms, int hidden, int bins) {
    if (!nsf_supported(dims, hidden, bins) || n_transforms < 1) {
        asmc_set_error("asmc_nsf_pack_floats: unsupported flow (1 <= dims <= 32, hidden in {32, 64}, bins = 8)");
        return ASMC_ERR_UNSUPPORTED;
    }
    const int ncg = nsf_ncg(dims);
    return hidden == 32 ? (int64_t)n_transforms * (Nsf<32>::bias(ncg) + Nsf<32>::layer_a(ncg))
                        : (int64_t)n_transforms * (Nsf<64>::bias(ncg) + Nsf<64>::layer_a(ncg));
}

extern "C" int asmc_nsf_pack(int dims, int n_transforms, int hidden, int bins, const float* const* weights_host,
                             const float* const* biases_host, float* packed_host) {
    ASMC_REQUIRE(weights_host && biases_host && packed_host, "null pointer");
    if (!nsf_supported(dims, hidden, bins) || n_transforms < 1) {
        asmc_set_error("asmc_nsf_pack: unsupported flow (1 <= dims <= 32, hidden in {32, 64}, bins = 8)");
        return ASMC_ERR_UNSUPPORTED;
    }
    return hidden == 32 ? nsf_pack_w<32>(dims, n_transforms, weights_host, biases_host, packed_host)
                        : nsf_pack_w<64>(dims, n_transforms, weights_host, biases_host, packed_host);
}

static int nsf_check(const char* who, const asmc_coupling* f) {
    if (!nsf_supported(f->dims, f->hidden, f->reserved) || f->n_layers < 1) {
        asmc_set_error("%s: unsupported spline flow (1 <= dims <= 32, hidden in {32, 64}, bins = 8 in the struct's reserved word)", who);
        return ASMC_ERR_UNSUPPORTED;
    }
    if (!asmc_flow_math_split()) {
        asmc_set_error("%s: spline flows run the split-fp16 layers only (ASMC_FLOW_MATH=f32 is not available there)", who);
        return ASMC_ERR_UNSUPPORTED;
    }
    return ASMC_OK;
}

template <int W, int NCG>
static size_t nsf_lds(int n_layers) { return (size_t)(2 * Nsf<W>::CW + n_layers * Nsf<W>::bias(NCG) + 96) * sizeof(float); }

template <class K>
static int nsf_raise_lds(asmc_ctx* ctx, K kern, size_t lds, size_t* attr_lds_dev) {
    size_t& attr_lds = attr_lds_dev[asmc_dev_slot(ctx)];
    if (lds > 64 * 1024 && lds > attr_lds) {
        ASMC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_lds = lds;
    }
    return ASMC_OK;
}

template <int W, int NCG, typename XT>
static int launch_nsf_logprob(asmc_ctx* ctx, int64_t n, const XT* x, const asmc_coupling* f, double* out, hipStream_t st) {
    constexpr int G = NSF_G_LOGPROB;
    const size_t lds = nsf_lds<W, NCG>(f->n_layers);
    ASMC_REQUIRE(lds <= 160 * 1024, "spline flow: the transforms' biases exceed the LDS");
    auto kern = k_nsf_logprob<W, NCG, XT, G>;
    static size_t attr_lds_dev[ASMC_MAX_DEVICES] = {0};  // per instantiation
    const int rc = nsf_raise_lds(ctx, kern, lds, attr_lds_dev);
    if (rc) return rc;
    const int64_t per_block = (int64_t)(NSF_THREADS / 64) * G * 16;
    const int64_t want = (n + per_block - 1) / per_block;
    const int grid = (int)(want < (int64_t)ctx->num_cu ? want : (int64_t)ctx->num_cu);  // one block per CU (registers)
    const float ladj0 = (float)(-f->log_scale_sum);
    const float base_const = (float)(-0.5 * f->dims * 1.8378770664093453);  // -d/2 log(2 pi)
    ASMC_LAUNCH(ctx, st, "k_nsf_logprob", kern, dim3(grid), dim3(NSF_THREADS), lds, st, n, (int)f->dims, x, f->packed_dev, (int)f->n_layers,
                f->loc_dev, f->scale_dev, ladj0, base_const, out);
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

template <int W, int NCG, typename XT>
static int launch_nsf_sample(asmc_ctx* ctx, int64_t n, const asmc_coupling* f, unsigned long long seed, unsigned long long gid0,
                             uint32_t draw_id, XT* x, double* out, hipStream_t st) {
    constexpr int G = NSF_G_SAMPLE;
    const size_t lds = nsf_lds<W, NCG>(f->n_layers);
    ASMC_REQUIRE(lds <= 160 * 1024, "spline flow: the transforms' biases exceed the LDS");
    auto kern = k_nsf_sample<W, NCG, XT, G>;
    static size_t attr_lds_dev[ASMC_MAX_DEVICES] = {0};  // per instantiation
    const int rc = nsf_raise_lds(ctx, kern, lds, attr_lds_dev);
    if (rc) return rc;
    const int64_t per_block = (int64_t)(NSF_THREADS / 64) * G * 16;
    const int64_t want = (n + per_block - 1) / per_block;
    const int grid = (int)(want < (int64_t)ctx->num_cu ? want : (int64_t)ctx->num_cu);
    const float ladj0 = (float)(-f->log_scale_sum);
    const float base_const = (float)(-0.5 * f->dims * 1.8378770664093453);
    ASMC_LAUNCH(ctx, st, "k_nsf_sample", kern, dim3(grid), dim3(NSF_THREADS), lds, st, n, (int)f->dims, f->packed_dev, (int)f->n_layers,
                f->loc_dev, f->scale_dev, ladj0, base_const, seed, gid0, draw_id, x, out,
                getenv("ASMC_NSF_SAMPLE_ALL_PASSES") ? 1 : 0);  // (diagnostic: the d-pass loop without the fixed-point exit)
    ASMC_LAUNCH_CHECK();
    return ASMC_OK;
}

#define NSF_SHAPES(X) X(32, 1) X(32, 2) X(64, 1) X(64, 2)

int asmc_nsf_logprob(asmc_ctx* ctx, int64_t n, int x_dtype, const void* x, const asmc_coupling* f, double* out, hipStream_t st) {
    const int rc = nsf_check("asmc_coupling_logprob", f);
    if (rc) return rc;
    const int ncg = nsf_ncg(f->dims);
#define X(WW, NN)                                                                                                        \
    if (f->hidden == WW && ncg == NN) {                                                                                  \
        if (x_dtype == ASMC_F64) return launch_nsf_logprob<WW, NN, double>(ctx, n, (const double*)x, f, out, st);       \
        if (x_dtype == ASMC_F32) return launch_nsf_logprob<WW, NN, float>(ctx, n, (const float*)x, f, out, st);         \
    }
    NSF_SHAPES(X)
#undef X
    asmc_set_error("asmc_coupling_logprob: bad x_dtype");
    return ASMC_ERR_ARG;
}

int asmc_nsf_sample(asmc_ctx* ctx, int64_t n, int x_dtype, const asmc_coupling* f, unsigned long long seed, unsigned long long gid0,
                    uint32_t draw_id, void* x_out, double* lq_out, hipStream_t st) {
    const int rc = nsf_check("asmc_coupling_sample", f);
    if (rc) return rc;
    const int ncg = nsf_ncg(f->dims);
#define X(WW, NN)                                                                                                                      \
    if (f->hidden == WW && ncg == NN) {                                                                                                \
        if (x_dtype == ASMC_F64) return launch_nsf_sample<WW, NN, double>(ctx, n, f, seed, gid0, draw_id, (double*)x_out, lq_out, st); \
        return launch_nsf_sample<WW, NN, float>(ctx, n, f, seed, gid0, draw_id, (float*)x_out, lq_out, st);                            \
    }
    NSF_SHAPES(X)
#undef X
    asmc_set_error("asmc_coupling_sample: unsupported spline flow shape");
    return ASMC_ERR_UNSUPPORTED;
}
