"""Host restatement of the tempered log-weights, their log-sum-exp reductions, ESS, the evidence moments, the normalised weights
and the adaptive-temperature search (csrc/asmc_weights.hip, csrc/asmc_search.hip, csrc/asmc_is_weights.hip, csrc/asmc_bisect.h), in numpy fp64 and numpy long double.

What is restated (reference paths relative to its root; no program text taken from it): samples.py:1221-1249 and :1276-1277 (the
log-weights, the evidence ratio and its variance, the normalised weights), utils.py:248-255 (log-sum-exp: maximum, then the sum of
exp(x - max)), utils.py:510-512 (ESS = exp(2 lse(x) - lse(2 x))) and samplers/smc/base.py:167-186 (the bisection of [beta0, 1]).

* `log_weights` is the fp64 specification: lw = fl(fl((beta0 - beta) lq) + fl((beta - beta0) fl(ll + lp))).  The kernels are compiled
  without contraction, so k_weights_map<0> and the maxima are held to it bit for bit, non-finite pattern included.
* The reductions take that fp64 lw (the argument of every exponential of the DIRECT kernels is fixed in fp64 by the
  specification) and sum in long double.  Each returns its value and the tolerance, built from the magnitudes of its terms.
* The PROGRESSION kernels (k_bis_sums, k_is_weights, k_bis_decide) are compared with long-double sums of the EXACT log-weight of
  the fp64 inputs, (beta - beta0) (ll + lp - lq), at the node's float and the kernel's shift m_j = fl(m(1) fl(fl(beta_j - beta0)
  fl(1 / (1 - beta0)))) (`node_shift`).

Tolerances (u = 2^-53; none comes from a device output):

  direct sums     S1: (L u + E) sum e_i;   S2: (L u + 2 E + u) sum e_i^2;   L = `chain_len`, the longest addition chain of the
                  dispatch: per-lane trips (n over grid x 256), 6 butterfly steps, 3 adds over the four waves, the finalize
                  kernel's ceil(grid / 64) strided adds and its 6 butterfly steps.
  m2              sum of 2 |d_i| (E e_i + u |d_i|) + (L + 1) u d_i^2 over the particles, d_i = e_i - mean_u.
  weights         w_i (E + u (|lw_i + shift| + |a_i| + 3 (|mp| + log N) + |lse| + 4) + tol(S1') / S1'), a_i the argument of the
                  exponential (+ one spacing of the subnormals, `SUBNORMAL_FLOOR`): the value of `shift` cancels; what stays are the roundings of
                  lw_i + shift and of the subtraction, those of lse = mp + log S1' (operands |mp| and log N, S1' = N up to
                  rounding), and the same roundings inside the terms that carry S1'.
  progression     per particle, relative: u (8 t (|lq_i| + |ll_i + lp_i|) + |lw_i| + 4 |lw_i - m|) + 6 u |m| + (15 + L) u + 2 E with
                  t = beta - beta0.  Derivation: the first exponential is the reference's expression at the lowest candidate,
                  beta_1 <= beta, so its roundings u (|c1 lq| + 2 |c2 (ll + lp)| + |lw| + |lw - m_1|) are bounded by those at
                  beta; the ratio's argument h ((ll + lp - lq) - Dmax) carries u h (|ll + lp| + |D_i| + 2 |D_i - Dmax|), raised
                  to a power j with j h <= t; the candidates' floats differ from beta_1 + j h and the closed-form shifts
                  from m_1 + j h Dmax by a few u t and u |m|: folded into the factors 8 and 6.  On top, (LU + 1) u (|D_i - Dmax| +
                  |Dmax|): the grid's floats are rounded midpoints of rounded midpoints, up to LU u / 2 off their dyadic points
                  in ABSOLUTE terms (LU = the level of the grid: 4 in the first round, hence for the sums at beta = 1, and the depth the
                  search reaches, `search_levels`, for a later round's), while the progression walks in exact
                  steps from its first node's float.  S2 doubles every share (+ u).
  block rescale   (k_is_weights round 0, k_bis_decide round 0) for a block / rank with maximum m_b under the merged M:
                  additionally u (2 |m_b - M| + 4 (|m_b| + |M|) + 12) + 32 E, weighted by that block's share of the sum (one
                  exponential of (m_b - M) / 16 - or of pw (m_b t - M t) - and an integer power up to 32).

E = `EXP_REL`: the device exp's relative error.  Measured on an MI355X against long double over every argument the cases of
tests/test_gpu_weights.py produce (k_weights_map<1> with shift = lse = 0): worst 0.86 ulp = 1.72 u; E is twice that.

The sequential search (`search`) returns beta* and the smallest |ESS/N - target| over the nodes it visited, in units of that
node's ESS tolerance (2 tol(S1) / S1 + tol(S2) / S2 of the progression form, times ESS/N).  A case is DECIDABLE when that margin is above 4
in the fp64 run and in the long-double run and both return the same beta*.

A test helper: the product never imports it.
"""
from __future__ import annotations

import math

import numpy as np

from transform_ref import LD, gap_ulps, same_nonfinite, ulp64  # noqa: F401  (re-exported for the tests)

U = 2.0 ** -53
EXP_ULPS_MEASURED = 0.86  # worst |device exp - long double| in ulps of the result over the suite's arguments (MI355X)
EXP_REL = 2.0 * (2.0 * EXP_ULPS_MEASURED * U)  # twice the worst seen (the sample is finite), as a relative error
# A subnormal result is a normal one (rounded once) scaled down and rounded again: half a spacing of the subnormals for each of the
# two roundings, whatever the relative error of the normal result.  For the weights that underflow this floor IS the error, so they sit
# near half of it; no other share can be reached exactly (each is an upper bound of an independent rounding).
SUBNORMAL_FLOOR = LD(2) ** -1074
BLOCK = 256
SCAN_TILE = 2048
ISW_CHUNK = 4096
MAX_BLOCKS = 2048


# ---- dispatch geometry (csrc/asmc_common.h reduce_grid, grid_for) -------------------------------------------------------------
def bucket_of(K):
    kt = 1
    while kt < K:
        kt <<= 1
    return kt


def reduce_grid(n, num_cu, kt=1):
    per_block = BLOCK * (4 if kt >= 16 else 8)
    cap = min(num_cu * 4, MAX_BLOCKS)
    return max(1, min((n + per_block - 1) // per_block, cap))


def chain_len(n, num_cu, kt=1):
    """Longest addition chain of the direct reductions: per-lane trips, wave butterfly, four waves, fixed-order finalize."""
    grid = reduce_grid(n, num_cu, kt)
    trips = (n + grid * BLOCK - 1) // (grid * BLOCK)
    return trips + 6 + 3 + (grid + 63) // 64 + 6


def bis_chain_len(n, num_cu):
    """k_bis_sums / k_is_weights: two adds per trip of 512 threads x grid, 6 butterfly steps, 7 adds over the eight waves, the
    record reduction (sixteen records per thread and pass, sixteen parts)."""
    grid = max(1, min((n + 511) // 512, num_cu))
    trips = (n + grid * 512 - 1) // (grid * 512)
    return trips + 6 + 7 + 16 * ((grid + 255) // 256) + 16


# ---- the fp64 specification ---------------------------------------------------------------------------------------------------------
def log_weights(ll, lp, lq, beta0, beta, shift=None):
    """lw in the reference's fp64 operation order (+ shift: SMCSamples.log_weights)."""
    ll, lp, lq = (np.asarray(a, dtype=np.float64) for a in (ll, lp, lq))
    with np.errstate(all="ignore"):
        c1, c2 = np.float64(beta0) - np.float64(beta), np.float64(beta) - np.float64(beta0)
        lw = c1 * lq + c2 * (ll + lp)
        return lw if shift is None else lw + np.float64(shift)


def lw_exact(ll, lp, lq, beta0, beta):
    """The exact log-weight of the fp64 inputs, (beta - beta0) (ll + lp - lq), in long double (non-finite rows as in fp64)."""
    with np.errstate(all="ignore"):
        t = LD(beta) - LD(beta0)
        return t * ((LD(1) * np.asarray(ll, dtype=LD) + np.asarray(lp, dtype=LD)) - np.asarray(lq, dtype=LD))


def max_and_nan(lw):
    """(maximum over the non-NaN entries, -inf when there is none; number of NaN entries): k_weights_max."""
    nan = np.isnan(lw)
    rest = lw[~nan]
    return (float(rest.max()) if rest.size else -math.inf), int(nan.sum())


def node_shift(m_one, beta, beta0):
    """The closed-form shift of a search node (bis_tail_core), in its fp64 operation order."""
    with np.errstate(all="ignore"):
        inv = np.float64(1.0) / (np.float64(1.0) - np.float64(beta0))
        return float(np.float64(m_one) * ((np.float64(beta) - np.float64(beta0)) * inv))


def bis_node_beta(K, LU, beta0):
    """The float the reference's loop holds for the dyadic node K / 2^LU of [beta0, 1] (asmc_bisect.h)."""
    if K <= 0:
        return float(beta0)
    if K >= (1 << LU):
        return 1.0
    lo, hi = np.float64(beta0), np.float64(1.0)
    mid = np.float64(0.5) * (hi + lo)
    tz = (K & -K).bit_length() - 1
    lev, k = LU - tz, K >> tz
    for b in range(lev - 1, 0, -1):
        if (k >> b) & 1:
            lo = mid
        else:
            hi = mid
        mid = np.float64(0.5) * (hi + lo)
    return float(mid)


def units(got, ref, tol):
    """Worst |got - ref| in units of tol over the elements (0 / 0 counts as 0: an exact result under a zero tolerance)."""
    with np.errstate(all="ignore"):
        err = np.abs(np.asarray(got, dtype=LD) - np.asarray(ref, dtype=LD))
        tol = np.asarray(tol, dtype=LD) + np.zeros_like(err)
        q = np.where(err == 0, LD(0), err / tol)
    return float(np.max(q)) if q.size else 0.0


# ---- reductions in long double -------------------------------------------------------------------------------------------------------
def _exp_ld(t):
    with np.errstate(all="ignore"):
        return np.exp(np.asarray(t, dtype=LD))


def sums(lw, m, shift=0.0, L=16, counts=None):
    """(S1, S2, tol1, tol2) of k_weights_sums: t = fl(fl(lw + shift) - m) in fp64, the exponentials and sums in long double.
    `counts`: multiplicities of the rows of lw (a large population built from few distinct rows: the same sums, cheaply)."""
    with np.errstate(all="ignore"):
        t = (np.asarray(lw, dtype=np.float64) + np.float64(shift)) - np.float64(m)
    e = _exp_ld(t)
    c = LD(1) if counts is None else np.asarray(counts, dtype=LD)
    with np.errstate(all="ignore"):
        S1, S2 = (c * e).sum(), (c * e * e).sum()
    return S1, S2, (L * U + EXP_REL) * S1, (L * U + 2 * EXP_REL + U) * S2


def ess_ld(S1, S2):
    with np.errstate(all="ignore"):
        return S1 * S1 / S2


def ess_tol(S1, S2, t1, t2):
    """Tolerance of S1^2 / S2 from those of the sums (first order)."""
    with np.errstate(all="ignore"):
        return ess_ld(S1, S2) * (2 * t1 / S1 + t2 / S2)


def evidence_ratio(m, S1, n):
    """log-sum-exp - log N (samples.py:1226-1228) from the triple, long double."""
    with np.errstate(all="ignore"):
        return LD(m) + np.log(LD(S1)) - np.log(LD(n))


def m2_lse(lw, m, mean_u, shift, mp, L=16, counts=None, free_shift=False):
    """k_weights_m2(_lse): (sum (exp(lw - m) - mean_u)^2, S1' = sum exp((lw + shift) - mp), tol_m2, tol_S1')."""
    lw = np.asarray(lw, dtype=np.float64)
    with np.errstate(all="ignore"):
        e = _exp_ld(lw - np.float64(m))
        d = e - LD(mean_u)
        c = LD(1) if counts is None else np.asarray(counts, dtype=LD)
        m2 = (c * d * d).sum()
        tol_m2 = (c * (2 * np.abs(d) * (EXP_REL * e + U * np.abs(d)) + (L + 1) * U * d * d)).sum()
        S1p, _, tol1, _ = sums(lw, mp, shift, L, counts)
        if free_shift:
            # shift and mp were formed on the device (its log): their value cancels, the roundings of lw + shift and of the
            # subtraction do not - 2 u (|lw + shift| + |(lw + shift) - mp| + |mp|) per term
            a = (lw + np.float64(shift)) - np.float64(mp)
            r = np.where(np.isfinite(a), 2 * U * (np.abs(lw + np.float64(shift)) + np.abs(a) + abs(mp)), 0.0)
            tol1 = tol1 + (c * _exp_ld(a) * r.astype(LD)).sum()
    return m2, S1p, tol_m2, tol1


def evidence_variance(m2, S1, n):
    """var_w / (N mean_w^2) (samples.py:1230-1242) from the device's moments: var = m2 / N, mean = S1 / N."""
    return (LD(m2) / LD(n)) / (LD(n) * (LD(S1) / LD(n)) ** 2)


def normalized_weights(ll, lp, lq, beta0, beta, L=16):
    """(w, tol): the true normalised weights of the fp64 log-weights, exp(lw_i) / sum exp(lw), in long double, and the elementwise
    tolerance of the device form exp(fl(fl(lw + shift) - lse)), lse = fl(mp + log S1'), mp = fl(m + shift), shift = fl(fl(m + log S1)
    - log N)."""
    lw = log_weights(ll, lp, lq, beta0, beta)
    m, _ = max_and_nan(lw)
    n = lw.size
    with np.errstate(all="ignore"):
        e = np.exp(lw.astype(LD) - LD(m))  # (the subtraction in long double too: the truth carries no fp64 rounding of its own)
        S1 = e.sum()
        t1 = (L * U + EXP_REL) * S1
        w = e / S1
        shift = float((np.float64(m) + np.log(np.float64(S1))) - np.log(np.float64(n)))
        mp = m + shift
        lse = mp + math.log(n)  # S1' = N up to rounding
        a = (lw + shift) - lse
        rel = EXP_REL + U * (np.abs(lw + shift) + np.abs(a) + 3 * (abs(mp) + math.log(n)) + abs(lse) + 4) + float(t1 / S1)
        tol = w * np.where(np.isfinite(rel), rel, 0.0).astype(LD) + SUBNORMAL_FLOOR
    return w, tol


# ---- the progression form ---------------------------------------------------------------------------------------------------------------
def search_levels(beta0, tol):
    """Depth of the dyadic grid a search on [beta0, 1] with tolerance tol reaches (asmc_bisect.h LU; one level of slack)."""
    if tol is None or not (1.0 - beta0 > tol):
        return 4
    return max(4, math.ceil(math.log2((1.0 - beta0) / tol)) + 1)


def progression_rel(ll, lp, lq, beta0, beta, m, L, block_m=None, M=None, tol_beta=None):
    """Per-particle relative tolerance of a progression term at node `beta` with shift `m` (module docstring).  `block_m`: the
    particle's block / rank maximum when the sums were first taken against it and rescaled to the merged maximum M."""
    # (k_bis_decide forms its factor as exp(pw (fl(m_r t) - fl(M t))): the two products' roundings, 4 u (|m_r| + |M|), on top)
    ll, lp, lq = (np.asarray(a, dtype=np.float64) for a in (ll, lp, lq))
    with np.errstate(all="ignore"):
        t = abs(float(beta) - float(beta0))
        ab = ll + lp
        lw = t * (ab - lq)
        rel = U * (8 * t * (np.abs(lq) + np.abs(ab)) + np.abs(lw) + 4 * np.abs(lw - m)) + 6 * U * abs(m) + (15 + L) * U + 2 * EXP_REL
        # the grid's floats: a node at level l is the rounded midpoint of rounded midpoints, up to l u / 2 off its dyadic
        # point (an ABSOLUTE error: the floats next to 1 are 2 u apart however small 1 - beta0 is).  The progression walks
        # from the first node's float in exact steps, the truth sits at the node's own float and the reported shift is
        # formed from it: up to (LU + 1) u between the two, times D_i - Dmax in the term and Dmax in the shift
        dmax = np.float64(m) / np.float64(t) if (t > 0 and math.isfinite(m)) else np.float64(0.0)
        d = (ab - lq) - dmax
        rel = rel + (search_levels(beta0, tol_beta) + 1) * U * (np.where(np.isfinite(d), np.abs(d), 0.0) + abs(dmax))
        if block_m is not None:
            bm = np.where(np.isfinite(block_m), block_m, M)
            rel = rel + U * (2 * np.abs(bm - M) + 4 * (np.abs(bm) + abs(M)) + 12) + 32 * EXP_REL
    return rel


def progression_sums(ll, lp, lq, beta0, beta, m, L, block_m=None, M=None, tol_beta=None):
    """(S1, S2, tol1, tol2): long-double sums of exp(lw_exact - m) at the node's float and their progression tolerances."""
    lw = lw_exact(ll, lp, lq, beta0, beta)
    with np.errstate(all="ignore"):
        e = np.exp(lw - LD(m))
        rel = progression_rel(ll, lp, lq, beta0, beta, m, L, block_m, M, tol_beta)
        relf = np.where(e > 0, rel, 0.0).astype(LD)  # (a zero term stays zero whatever its magnitudes)
        S1, S2 = e.sum(), (e * e).sum()
        t1, t2 = (e * relf).sum(), (e * e * (2 * relf + U)).sum()
    return S1, S2, t1, t2


def emulate_round(ll, lp, lq, c1, c2, m1, h, dmax, order=None):
    """numpy fp64 emulation of one k_bis_sums round: two exponentials per particle and fifteen multiplications; S1[16], S2[16] in
    ascending candidate order.  `order`: a permutation of the particles (the sum's order)."""
    ll, lp, lq = (np.asarray(a, dtype=np.float64) for a in (ll, lp, lq))
    if order is not None:
        ll, lp, lq = ll[order], lp[order], lq[order]
    with np.errstate(all="ignore"):
        e = np.exp((c1 * lq + c2 * (ll + lp)) - m1)
        r = np.exp(h * (((ll + lp) - lq) - dmax))
        S1, S2 = np.empty(16), np.empty(16)
        for j in range(16):
            S1[j], S2[j] = e.sum(), (e * e).sum()
            e = e * r
    return S1, S2


def first_round_grid(beta0, m_one):
    """(c1, c2, m1, h, dmax) of the first round (k_bis_sums round 0), fp64 operation order."""
    lo = np.float64(beta0)
    b1 = np.float64(1.0)
    for _ in range(4):
        b1 = np.float64(0.5) * (b1 + lo)
    with np.errstate(all="ignore"):
        inv = np.float64(1.0) / (np.float64(1.0) - lo)
        return lo - b1, b1 - lo, np.float64(m_one) * ((b1 - lo) * inv), (np.float64(1.0) - lo) / np.float64(16.0), np.float64(m_one) * inv


def int_pow(base, e0):
    """base^e0 by the kernel's binary powering (six squarings, a multiplication per set bit), fp64."""
    f, pw = np.ones_like(base), base.copy()
    for bit in range(6):
        if (e0 >> bit) & 1:
            f = f * pw
        pw = pw * pw
    return f


def emulate_round0_blocks(ll, lp, lq, beta0, chunk=ISW_CHUNK, rescale=True, dead_block_m="M"):
    """numpy fp64 emulation of k_is_weights' first round: every chunk reduced against its OWN maximum, the records rescaled to the
    merged one by exp((m_b - M) / 16)^(pw ks).  Returns (S1[16], S2[16], M, block maxima).  rescale=False and dead_block_m="0"
    are two of the mistakes tests/test_weights_ref.py plants."""
    n = len(ll)
    lw1 = log_weights(ll, lp, lq, beta0, 1.0)
    nb = (n + chunk - 1) // chunk
    mb = np.array([max_and_nan(lw1[b * chunk:(b + 1) * chunk])[0] for b in range(nb)])
    # a block without a finite log-weight counts as m_b = M: it takes no part in the merged maximum (the planted mistake: as 0)
    M = float(mb.max()) if dead_block_m == "M" else float(np.where(mb > -math.inf, mb, 0.0).max())
    S1, S2 = np.zeros(16), np.zeros(16)
    for b in range(nb):
        sl = slice(b * chunk, (b + 1) * chunk)
        m_block = mb[b] if mb[b] > -math.inf else 0.0
        s1, s2 = emulate_round(ll[sl], lp[sl], lq[sl], *first_round_grid(beta0, m_block))
        with np.errstate(all="ignore"):
            if mb[b] > -math.inf and M > -math.inf:
                base = np.array([math.exp((mb[b] - M) * (1.0 / 16.0))])
            else:
                base = np.array([1.0])
            for ks in range(1, 17):
                f1, f2 = (int_pow(base, ks)[0], int_pow(base, 2 * ks)[0]) if rescale else (1.0, 1.0)
                S1[ks - 1] += s1[ks - 1] * f1
                S2[ks - 1] += s2[ks - 1] * f2
    return S1, S2, M, mb


# ---- the sequential search ---------------------------------------------------------------------------------------------------------------
def _eff_f64(ll, lp, lq, beta0, beta):
    """ESS/N with the reference's fp64 expressions (log_weights, then exp(2 lse(x) - lse(2 x)))."""
    lw = log_weights(ll, lp, lq, beta0, beta)
    n = lw.size
    with np.errstate(all="ignore"):
        def lse(x):
            c = x.max()
            return c + np.log(np.sum(np.exp(x - c)))
        x = lw + (lse(lw) - math.log(n))
        return float(np.exp(lse(x) * 2 - lse(x * 2))) / n


def _eff_ld(ll, lp, lq, beta0, beta):
    lw = lw_exact(ll, lp, lq, beta0, beta)
    with np.errstate(all="ignore"):
        e = np.exp(lw - lw.max())
        return (e.sum() ** 2 / (e * e).sum()) / LD(lw.size)


def eff_tolerance(ll, lp, lq, beta0, beta, m_one, L, tol_beta=None):
    """Tolerance of ESS/N at a search node, from the progression tolerances of its sums.  (Magnitudes only: formed in fp64.)"""
    m = node_shift(m_one, beta, beta0)
    ll, lp, lq = (np.asarray(a, dtype=np.float64) for a in (ll, lp, lq))
    with np.errstate(all="ignore"):
        e = np.exp((float(beta) - float(beta0)) * ((ll + lp) - lq) - m)
        rel = np.where(e > 0, progression_rel(ll, lp, lq, beta0, beta, m, L, tol_beta=tol_beta), 0.0)
        S1, S2 = e.sum(), (e * e).sum()
        return float((S1 * S1 / S2) * (2 * (e * rel).sum() / S1 + (e * e * (2 * rel + U)).sum() / S2) / len(ll))


def search(ll, lp, lq, beta0, target, tol, ft=np.float64, L=64):
    """The reference's loop.  Returns (beta*, margin, n_nodes): margin = min over the visited nodes of |ESS/N - target| in units of
    the node's ESS tolerance (inf when no node was visited or a node's ESS is NaN, which compares false whatever the rounding)."""
    eff_fn = _eff_f64 if ft is np.float64 else _eff_ld
    m_one, _ = max_and_nan(log_weights(ll, lp, lq, beta0, 1.0))
    margin, nodes = math.inf, 0

    def visit(beta):
        nonlocal margin, nodes
        eff = eff_fn(ll, lp, lq, beta0, beta)
        nodes += 1
        if eff == eff:
            et = eff_tolerance(ll, lp, lq, beta0, beta, m_one, L, tol)
            margin = min(margin, abs(float(eff) - target) / et if et > 0 else math.inf)
        return eff

    bmin, bmax = np.float64(beta0), np.float64(1.0)
    if visit(1.0) >= target:
        bmin = np.float64(1.0)
    while bmax - bmin > tol:
        mid = np.float64(0.5) * (bmax + bmin)
        if visit(float(mid)) >= target:
            bmin = mid
        else:
            bmax = mid
    return float(bmin), margin, nodes


def decide(ll, lp, lq, beta0, target, tol, L=64):
    """(beta*, decidable, margin) of a case: both runs, the margin rule of the module docstring."""
    b64, g64, _ = search(ll, lp, lq, beta0, target, tol, np.float64, L)
    bld, gld, _ = search(ll, lp, lq, beta0, target, tol, LD, L)
    return b64, (b64 == bld and g64 > 4 and gld > 4), min(g64, gld)


# ---- populations ------------------------------------------------------------------------------------------------------------------------
POPULATIONS = ("synth", "heavy", "peaked3e3", "peaked3e4", "dominant", "uniform", "neginf20", "neginf_chunk", "neginf_lanes",
               "plateau_above", "plateau_below", "offset1e3", "offset1e6", "sorted_up", "sorted_down")


def population(kind, n, seed=0):
    """(ll, lp, lq) of the named population (module docstring of tests/test_gpu_weights.py)."""
    g = np.random.default_rng([seed, POPULATIONS.index(kind) if kind in POPULATIONS else 99, n])
    if kind in ("synth", "offset1e3", "offset1e6", "sorted_up", "sorted_down"):
        x = 1.5 * g.normal(size=(n, 4))
        ll = -0.5 * np.sum(x ** 2, axis=1)
        lp = ll.copy()
        lq = -0.5 * np.sum((x / 1.5) ** 2, axis=1) - 4 * np.log(1.5) - 2 * np.log(2 * np.pi)
        if kind.startswith("offset"):
            off = 1e3 if kind == "offset1e3" else 1e6
            ll, lq = ll + off, lq + off
        if kind.startswith("sorted"):
            ll = ll * 60.0  # block maxima hundreds apart
            o = np.argsort((ll + lp) - lq)
            o = o if kind == "sorted_up" else o[::-1]
            ll, lp, lq = ll[o].copy(), lp[o].copy(), lq[o].copy()
    elif kind == "heavy":
        ll, lp, lq = g.standard_t(2, n) * 20.0, g.normal(size=n), g.normal(size=n)
    elif kind in ("peaked3e3", "peaked3e4"):
        ll, lp, lq = -np.abs(g.normal(size=n)) * (3e3 if kind == "peaked3e3" else 3e4), g.normal(size=n), g.normal(size=n) * 2
    elif kind == "dominant":
        ll, lp, lq = g.normal(size=n), g.normal(size=n), g.normal(size=n)
        ll[(n * 2) // 3] += 500.0
    elif kind == "uniform":
        ll, lp, lq = 1e-3 * g.normal(size=n), np.zeros(n), np.zeros(n)
    elif kind in ("neginf20", "neginf_chunk", "neginf_lanes", "neginf_all"):
        ll, lp, lq = g.normal(size=n), g.normal(size=n), g.normal(size=n)
        if kind == "neginf20":
            ll[g.uniform(size=n) < 0.2] = -np.inf
        elif kind == "neginf_chunk":  # the second 4096-chunk, whole (n <= 4096: the first half of the rows)
            ll[slice(4096, 8192) if n > 4096 else slice(0, n // 2)] = -np.inf
        elif kind == "neginf_lanes":  # the particles one wave of a 512-thread block sees at every stride of 512
            i = np.arange(n)
            ll[(i % 512) < 64] = -np.inf
        else:
            ll[:] = -np.inf
    elif kind in ("plateau_above", "plateau_below"):  # equal Delta: ESS/N = the finite fraction at every beta > beta0
        frac = 0.25 if kind == "plateau_above" else 0.75
        ll, lp, lq = np.full(n, 1.25), np.full(n, -0.5), np.full(n, 0.25)
        ll[: int(round(n * frac))] = -np.inf
    else:
        raise ValueError(kind)
    return ll, lp, lq


# ---- the non-finite contract -----------------------------------------------------------------------------------------------------------
NONFINITE_CLASSES = ("some_neginf", "all_neginf", "posinf_row", "inf_minus_inf_row", "nan_row")


def nonfinite_case(cls, n=300, seed=5):
    g = np.random.default_rng(seed)
    ll, lp, lq = g.normal(size=n), g.normal(size=n), g.normal(size=n)
    if cls == "some_neginf":
        ll[::3] = -np.inf
    elif cls == "all_neginf":
        ll[:] = -np.inf
    elif cls == "posinf_row":
        ll[n // 2] = np.inf
    elif cls == "inf_minus_inf_row":
        ll[n // 2], lq[n // 2] = np.inf, np.inf
    elif cls == "nan_row":
        lp[n // 2] = np.nan
    else:
        raise ValueError(cls)
    return ll, lp, lq


def nonfinite_contract(cls, beta0=0.0, beta=0.5, target=0.5, tol=1e-6, n=300, seed=5):
    """What the restated reference gives for the class: the row of the contract table.
    `raises`: SMCSamples.log_weights raises on a NaN log-weight (samples.py:1246-1247); the device reports the census instead and
    `found` is 0.  `beta_star == beta0` is where the reference's determine_beta raises its BetaScheduleError."""
    ll, lp, lq = nonfinite_case(cls, n, seed)
    lw = log_weights(ll, lp, lq, beta0, beta)
    m, n_nan = max_and_nan(lw)
    S1, S2, _, _ = sums(lw, m)
    with np.errstate(all="ignore"):
        ess = float(ess_ld(S1, S2))
    raises = n_nan > 0
    b_star = search(ll, lp, lq, beta0, target, tol)[0]
    found = (not raises) and b_star > beta0
    return dict(cls=cls, m=m, S1=float(S1), S2=float(S2), n_nan=n_nan, ess=ess, ratio=float(evidence_ratio(m, S1, n)),
                raises=raises, beta_star=b_star, found=found, weights="normalised" if found else "1/N")


# ---- the search cases shared by tests/test_weights_ref.py (decidability) and tests/test_gpu_weights.py ----------------------------
BETA0S = (0.0, 0.013, 0.4, 0.93, 1.0 - 2.0 ** -20, float(np.nextafter(1.0, 0.0)))
TOLS = (1e-3, 1e-6, 1e-8, 0.5, 2.0)
TARGETS = (0.3, 0.5, 0.9)
SEARCH_N = (1, 2, 3, 511, 513, 1025, 131071, 131073, 262145)
SEARCH_POPULATIONS = POPULATIONS + ("neginf_all",)


def named_search_cases():
    """(kind, n, seed, beta0, target, tol): every population, every beta0, tolerance, target and n of the issue at least once.
    None of them may be undecidable."""
    cases = [(k, 1025, 1, 0.0, 0.5, 1e-6) for k in SEARCH_POPULATIONS]
    cases += [(k, 513, 2, b0, 0.5, 1e-8) for k in ("synth", "heavy") for b0 in BETA0S]
    cases += [(k, 511, 3, 0.013, 0.3, tol) for k in ("synth", "neginf20") for tol in TOLS]
    cases += [("synth", 513, 4, 0.4, 0.5, 2.0), ("heavy", 513, 4, 0.93, 0.9, 0.5), ("plateau_below", 513, 4, 0.4, 0.5, 2.0)]
    cases += [(k, 1025, 5, 0.0, t, 1e-6) for k in ("synth", "peaked3e3") for t in TARGETS]
    cases += [(k, n, 6, 0.0, 0.5, 1e-6) for k in ("synth", "neginf20", "dominant") for n in SEARCH_N
              if n < 100000 and not (k == "dominant" and n < 3)]  # (two particles: ESS/N >= 1/2 = the target at every beta)
    cases += [(k, n, 6, 0.0, 0.5, 1e-6) for k in ("synth", "neginf_lanes") for n in SEARCH_N if n > 100000]
    return list(dict.fromkeys(cases))


def random_search_cases(count=100, seed=2026):
    g = np.random.default_rng(seed)
    kinds = ("synth", "heavy", "peaked3e3", "peaked3e4", "dominant", "uniform", "neginf20", "sorted_up")
    out = []
    for i in range(count):
        out.append((str(g.choice(kinds)), int(g.choice([3, 17, 64, 300, 511, 513, 1025, 2048, 5000])), 100 + i,
                    float(g.choice(BETA0S[:5])), float(g.choice(TARGETS)), float(g.choice([1e-3, 1e-6, 1e-8]))))
    return out


_DECIDED = {}


def decide_cached(key, ll, lp, lq, beta0, target, tol, L=64):
    """`decide` of a population that is not one of `population`'s, computed once per process under `key`."""
    if key not in _DECIDED:
        _DECIDED[key] = decide(ll, lp, lq, beta0, target, tol, L)
    return _DECIDED[key]


def plain_levels(beta0, tol):
    """Iterations of the reference's loop: halvings of 1 - beta0 until the bracket is within the tolerance."""
    w, k = np.float64(1.0) - np.float64(beta0), 0
    while w > tol:
        w, k = w * 0.5, k + 1
    return k


def decided(case, L=64):
    """`decide` of a search case, computed once per process."""
    if case not in _DECIDED:
        kind, n, seed, beta0, target, tol = case
        _DECIDED[case] = decide(*population(kind, n, seed), beta0, target, tol, L)
    return _DECIDED[case]


def later_round_grid(beta0, m_one, K_first, stride, LU):
    """(c1, c2, m1, h, dmax) of a later round on the nodes K_first + j stride of level LU (asmc_bisect.h bis_plan's last lines)."""
    with np.errstate(all="ignore"):
        b0 = np.float64(beta0)
        inv = np.float64(1.0) / (np.float64(1.0) - b0)
        bf = np.float64(bis_node_beta(K_first, LU, beta0))
        return (b0 - bf, bf - b0, np.float64(m_one) * ((bf - b0) * inv), (np.float64(1.0) - b0) * np.float64(math.ldexp(float(stride), -LU)),
                np.float64(m_one) * inv)
