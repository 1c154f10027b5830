// asmc_nsf_dev.h — the monotonic rational-quadratic spline of the neural spline flow (include/asmc.h ASMC_FLOW_NSF;
// aspire_amd/flows.py NSFFlow / _SplineAutoregressive), one coordinate at a time, lane local.
//
// Reference: examples/smc_example.py:82 asks zuko for flow_class="NSF" (flows/torch/flows.py:155-164 forwards the name); zuko
// is absent, so this is the repository's statement of its documented MonotonicRQSTransform (bound 5, slope 1e-3), UNVERIFIED
// against the package.  With c = ln 1000, K = 8 bins, B = 5:
//   w <- w / (1 + 2 |w| / c), h likewise, delta <- delta / (1 + |delta| / c)
//   X_0 = -B, X_j = B (2 sum_{m <= j} softmax(w)_m - 1), X_K = +B exactly (Y from h);  D_0 = D_K = 1, D_j = exp(delta_j)
//   k = #{j : X_j < x} - 1, inside <=> 0 <= k < K (x = -B is outside, x = +B the last bin at zeta = 1); outside: y = x, log J = 0
// Plain fp32 with correctly rounded divisions (the softmax is normalised by one rounded reciprocal per coordinate) and the
// library's expf / logf / sqrtf: the knots carry fp32 rounding into bins whose log J has curvature up to 1e4, so every ulp given
// away here is paid a thousandfold in the density.
// The functions compile for the host as well (a CPU check of the edges needs no GPU).
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define NSF_HD __host__ __device__ __forceinline__
#else
#define NSF_HD inline
#endif

#define NSF_BINS 8
#define NSF_PARAMS (3 * NSF_BINS - 1)
#define NSF_BOUND 5.0f
#define NSF_LN1000 6.907755278982137f

// the NSF_BINS - 1 interior knots of one coordinate from its raw widths (or heights)
NSF_HD void nsf_knots(const float (&raw)[NSF_BINS], float (&kn)[NSF_BINS - 1]) {
    float r[NSF_BINS], m = -INFINITY;
#pragma unroll
    for (int c = 0; c < NSF_BINS; c++) {
        r[c] = raw[c] / (1.0f + fabsf(raw[c]) * (2.0f / NSF_LN1000));
        m = fmaxf(m, r[c]);
    }
    float tot = 0.0f;
#pragma unroll
    for (int c = 0; c < NSF_BINS; c++) {
        r[c] = expf(r[c] - m);
        tot += r[c];
    }
    const float inv = 1.0f / tot;  // (one division per coordinate: a product with the rounded reciprocal is within an ulp of the quotient)
    float cs = 0.0f;
#pragma unroll
    for (int j = 0; j < NSF_BINS - 1; j++) {
        cs += r[j] * inv;
        kn[j] = NSF_BOUND * (2.0f * cs - 1.0f);
    }
}

// bin of v among the knots K_0 = -B, K_j = kn[j - 1], K_8 = +B: k = #{K_j < v} - 1 (-1 and NSF_BINS: outside; a NaN is
// outside), and the bin's two knots
NSF_HD void nsf_locate(const float (&kn)[NSF_BINS - 1], float v, int& k, float& lo, float& hi) {
    k = -1, lo = -NSF_BOUND, hi = -NSF_BOUND;
    float prev = -NSF_BOUND;
#pragma unroll
    for (int j = 1; j <= NSF_BINS; j++) {
        const float cur = j < NSF_BINS ? kn[j - 1] : NSF_BOUND;
        if (prev < v) k = j - 1, lo = prev, hi = cur;
        prev = cur;
    }
    if (NSF_BOUND < v) k = NSF_BINS;
}

// the two knots of bin k (0 <= k < NSF_BINS; anything else leaves lo = hi = -B, which the callers discard)
NSF_HD void nsf_bin_knots(const float (&kn)[NSF_BINS - 1], int k, float& lo, float& hi) {
    lo = -NSF_BOUND, hi = -NSF_BOUND;
    float prev = -NSF_BOUND;
#pragma unroll
    for (int j = 1; j <= NSF_BINS; j++) {
        const float cur = j < NSF_BINS ? kn[j - 1] : NSF_BOUND;
        if (k == j - 1) lo = prev, hi = cur;
        prev = cur;
    }
}

// the derivatives at the two knots of bin k from the NSF_BINS - 1 raw interior values (only the two that are needed are formed)
NSF_HD void nsf_bin_derivs(const float (&raw)[NSF_BINS - 1], int k, float& d0, float& d1) {
    float r0 = 0.0f, r1 = 0.0f;
#pragma unroll
    for (int j = 0; j < NSF_BINS - 1; j++) {
        if (k == j + 1) r0 = raw[j];
        if (k == j) r1 = raw[j];
    }
    d0 = (k >= 1 && k < NSF_BINS) ? expf(r0 / (1.0f + fabsf(r0) * (1.0f / NSF_LN1000))) : 1.0f;
    d1 = (k >= 0 && k < NSF_BINS - 1) ? expf(r1 / (1.0f + fabsf(r1) * (1.0f / NSF_LN1000))) : 1.0f;
}

NSF_HD bool nsf_inside(int k) { return k >= 0 && k < NSF_BINS; }

// log J of the data -> latent map at position zeta of a bin of slope s = ht / wd with knot derivatives d0, d1
NSF_HD float nsf_logj(float s, float zeta, float d0, float d1) {
    const float zz = zeta * (1.0f - zeta);
    const float q = s + (d0 + d1 - 2.0f * s) * zz;
    return logf(s * s * (2.0f * s * zz + d0 * (1.0f - zeta) * (1.0f - zeta) + d1 * zeta * zeta) / (q * q));
}

// data -> latent: x in bin k = [x0, x0 + wd] -> y in [y0, y0 + ht]; outside the box the identity
NSF_HD void nsf_forward(float x, int k, float x0, float wd, float y0, float ht, float d0, float d1, float& y, float& lj) {
    const float s = ht / wd;
    const float zeta = (x - x0) / wd;
    const float zz = zeta * (1.0f - zeta);
    const float q = s + (d0 + d1 - 2.0f * s) * zz;
    const float yy = y0 + ht * (s * zeta * zeta + d0 * zz) / q;
    const float l = nsf_logj(s, zeta, d0, d1);
    const bool in = nsf_inside(k);
    y = in ? yy : x;
    lj = in ? l : 0.0f;
}

// latent -> data (the bin was found on Y); lj is log J of the data -> latent map at the returned x
NSF_HD void nsf_inverse(float y, int k, float x0, float wd, float y0, float ht, float d0, float d1, float& x, float& lj) {
    const float s = ht / wd;
    const float eta = y - y0;
    const float t = d0 + d1 - 2.0f * s;
    const float a = ht * (s - d0) + eta * t;
    const float b = ht * d0 - eta * t;
    const float c2 = -s * eta;
    const float zeta = 2.0f * c2 / (-b - sqrtf(b * b - 4.0f * a * c2));
    const float l = nsf_logj(s, zeta, d0, d1);
    const bool in = nsf_inside(k);
    x = in ? x0 + zeta * wd : y;
    lj = in ? l : 0.0f;
}
