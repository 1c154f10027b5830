"""Plain restatement of the resampling operations of csrc/asmc_cdf.hip and csrc/asmc_resample.hip (no GPU, nothing imported from the code under test):
the judge of tests/test_gpu_resample.py, pinned by tests/test_resample_ref.py.  DESIGN.md section 3.17 has the path table.

  exact cdf            np.cumsum (sequential fp64): the device must give its bits
  fast cdf             the cumulative sum in long double and a tolerance derived from the kernel's additions (fast_tol)
  search               np.searchsorted(cdf, u, side="right"); the device's two pinned deviations are in `search_device`:
                       a NaN key gives 0 (no cdf[k] <= NaN; numpy sorts NaN last and answers n), and a key below 1 never gives n
  guide table          G[b] = #{k : cdf[k] <= b / nb}, b = 0 .. nb, and the bucket rule b / nb <= u < (b + 1) / nb, evaluated with
                       the same fp64 divisions as the kernels (`guide`, `bucket`); `guided_search` is the search inside the window
  PCG64                np.random.Generator(PCG64).random, offsets through `advance`
  systematic uniforms  ((j0 + j) + off) / n_total in fp64
  gather / compaction / range selection   numpy fancy and boolean indexing
  column-sum partials  the sum of the gathered rows in long double

Fast-cdf tolerance.  Every fast-cdf value is a sum of non-negative terms formed by a fixed tree of fp64 additions, possibly
replaced by another such value through a maximum or a clamp (exact operations).  A sum tree whose deepest leaf passes through A
additions carries a relative error of at most gamma_A = A u / (1 - A u), u = 2^-53, against the true sum of its leaves (all terms
are >= 0: no cancellation).  Counting the additions a weight passes through on its way into an element of tile b (thread = 8
consecutive weights, wave = 64 threads, tile = 4 waves = 2048 weights, chunk = 1024 tiles; an addition to 0.0 is exact):

  a weight of an earlier tile of the same chunk:
      k_tile_sum      7 (the thread's serial sum) + 6 (xor butterfly) + 3 (((s0 + s1) + s2) + s3)              = 16
      k_scan_tiles    6 (Hillis-Steele steps over the wave's tiles) + 15 (carry + the waves in front, serially)
                      + 1 (wave prefix + inclusive value; the exclusive prefix is the neighbour's inclusive one)  = 22
      k_tile_scan     3 (tile prefix + the waves in front) + 1 (+ the lanes in front) + 1 (+ the thread's own sum) = 5
                                                                                                          total   43
  every further chunk in front adds its hand-over: 15 + 1 = 16 more
  a weight of the same tile: 7 + 6 + 3 + 1 + 1 = 18 at most; of the same thread: 7 + 1 = 8

so A(n) = 43 + 16 (ceil(n_tiles / 1024) - 1).  The kernel has no subtraction: every exclusive prefix is the neighbour's
inclusive sum.  The maxima and clamps are exact operations that replace a value x (true value P_k) only by

  - the computed value x' > x of an EARLIER prefix (true value P' <= P_k):  P_k (1 - g) <= x < x' <= P' (1 + g) <= P_k (1 + g);
  - the tile's upper bound h < x, the computed prefix at the tile's end (true value S >= P_k; the total for the last tile):
    P_k (1 - g) <= S (1 - g) <= h < x <= P_k (1 + g);

with g = gamma_A, so the bound stays RELATIVE TO THE ELEMENT'S OWN true value everywhere:

  |cdf[k] - P_k| <= gamma_A P_k          (carry_in is part of P_k)

which is what keeps the small prefix in front of a dominant weight (`dominant`).  The group sum that scaled the tolerance while
the kernels took `inc - acc` (the true cumulative sum at the end of the thread, wave or tile whose inclusive sum was the
minuend) is `fast_tol(..., scale="tile")`, kept for the record of the parent's errors; the tests assert the tighter "own".
Normalised: x / T with T the device's total, itself within gamma_A of the truth, and one rounding of the division:
(2 gamma_A + 2 u) P_k / P_n.  The last element is the total bit for bit, and the normalised last element is exactly 1 (NaN when
the total is 0 or not finite).  The count comes from the kernel's code, not from its output.
"""
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
BLOCK = 256
SCAN_TILE = 2048
SCAN_CHUNK = 1024  # tiles per trip of k_scan_tiles
SEARCH_GUIDE_MIN_N = 1 << 17  # asmc_search builds the guide table from this n on ...
GATHER_PACK_MIN_N = 1 << 16   # ... asmc_gather packs (ll, lp, lq) records from this n_in on when n_out >= n_in / 4
MAX_BLOCKS = 2048

assert np.finfo(LD).nmant >= 63, "the restatement needs an extended long double"


# ---- weight laws ---------------------------------------------------------------------------------------------------------------------------
PARITY_LAWS = ("smooth", "heavy", "tiny_first", "equal", "ties")  # the five of tests/test_gpu_parity.py, restated
LAWS = PARITY_LAWS + ("zeros70", "dominant", "first_only", "last_only", "zeros_tail", "all_zero")


def dominant_index(n):
    """Where `dominant` puts its one large weight: the fourth of a thread's eight elements, in lane 37 of the wave that holds the
    middle of the population (lane 0 has no lanes in front: its exclusive prefix within the wave is 0 however it is formed)."""
    k = (n // 2) // 512 * 512 + 37 * 8 + 3
    return k if k < n else min((n // 2) // 8 * 8 + 3, n - 1)


def weights(law, n, seed=0):
    g = np.random.default_rng([seed, LAWS.index(law), n])
    if law == "smooth":
        w = np.exp(g.normal(size=n))
    elif law == "heavy":  # hundreds of binades, exact zeros, a dominant weight
        w = np.exp(60 * g.normal(size=n))
        w[g.integers(0, n, n // 10)] = 0.0
    elif law == "tiny_first":
        w = np.exp(g.normal(size=n))
        k = min(5, n)
        w[:k] = [0.0, 5e-324, 1e-310, 3e-300, 1e-200][:k]
        return w
    elif law == "equal":
        return np.full(n, 1.0 / n)
    elif law == "ties":  # dyadic weights: every addition is a candidate for a round-to-even tie
        w = np.ldexp(1.0, -g.integers(1, 60, n).astype(np.int64)).astype(np.float64)
    elif law == "zeros70":
        w = np.exp(g.normal(size=n))
        w[g.random(n) < 0.7] = 0.0
    elif law == "dominant":
        w = np.full(n, 1e-30)
        w[dominant_index(n)] = 1e30
        return w
    elif law == "first_only":
        w = np.zeros(n)
        w[0] = 0.75
        return w
    elif law == "last_only":
        w = np.zeros(n)
        w[-1] = 0.75
        return w
    elif law == "zeros_tail":
        w = np.exp(g.normal(size=n))
        w[max(1, n - 3000):] = 0.0
    elif law == "all_zero":
        return np.zeros(n)
    else:
        raise ValueError(law)
    s = w.sum()
    return w / s if s > 0 else w


# ---- cumulative sums -------------------------------------------------------------------------------------------------------------------------
def exact_cdf(w, carry=0.0, normalize=False):
    """numpy's sequential fp64 cumulative sum behind `carry`; normalize: divided by its last element (numpy's division)."""
    c = np.cumsum(np.concatenate([[np.float64(carry)], np.asarray(w, dtype=np.float64)]))[1:]
    with np.errstate(all="ignore"):
        return c / c[-1] if normalize else c


def fast_cdf(w, carry=0.0):
    """The prefix sums of the fp64 weights in long double, by blocks of 2048 (the blocks' sums accumulated separately), so that
    an element passes through at most 2048 + n / 2048 long-double additions: `REF_REL(n)` bounds the reference's own relative
    error, which `fast_tol` adds to the tolerance (3 % of it at n = 2^21 in the worst case)."""
    w = np.asarray(w, dtype=LD)
    n = w.size
    pad = (-n) % SCAN_TILE
    blocks = np.concatenate([w, np.zeros(pad, dtype=LD)]).reshape(-1, SCAN_TILE)
    inner = np.cumsum(blocks, axis=1)
    front = np.concatenate([[LD(carry)], LD(carry) + np.cumsum(inner[:-1, -1])])
    return (inner + front[:, None]).reshape(-1)[:n]


def REF_REL(n):
    return LD(SCAN_TILE + n // SCAN_TILE + 2) * LD(2) ** -64


def fast_additions(n):
    """A(n) of the module docstring: the additions on the deepest path into a fast-cdf element."""
    n_tiles = (n + SCAN_TILE - 1) // SCAN_TILE
    return 43 + 16 * ((n_tiles + SCAN_CHUNK - 1) // SCAN_CHUNK - 1)


def fast_tol(w, carry=0.0, normalize=False, scale="own"):
    """(reference, elementwise tolerance) of the fast cdf (module docstring).  scale = "own": the element's own true value;
    "tile": the true cumulative sum at the end of the element's tile (the looser bound of a scan that subtracts)."""
    P = fast_cdf(w, carry)
    n = P.size
    A = fast_additions(n)
    gam = LD(A * U) / (LD(1) - LD(A * U)) + REF_REL(n)
    if scale == "tile":
        ends = np.minimum((np.arange(n) // SCAN_TILE + 1) * SCAN_TILE, n) - 1
        S = P[ends]
    else:
        S = P
    # a rounding whose result is subnormal errs by up to half a spacing of the subnormals whatever the relative bound says
    floor = LD(A + 1) * LD(2) ** -1074
    if not normalize:
        return P, gam * S + floor
    with np.errstate(all="ignore"):
        return P / P[-1], (2 * gam + LD(2 * U)) * S / P[-1] + floor / P[-1] + floor


def units(got, ref, tol):
    """Worst |got - ref| in units of tol over the elements.  An exact match counts as 0 whatever the tolerance (0 / 0: an exact
    zero must be met exactly), NaN against NaN too; NaN against a number is inf."""
    got, ref = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD)
    with np.errstate(all="ignore"):
        err = np.abs(got - ref)
        q = np.where((err == 0) | (np.isnan(got) & np.isnan(ref)), LD(0), err / tol)
        q = np.where(np.isnan(q), LD(np.inf), q)
    return float(np.max(q)) if q.size else 0.0


# ---- search ----------------------------------------------------------------------------------------------------------------------------------
def search(cdf, u):
    """#{k : cdf[k] <= u}: numpy's searchsorted, side="right" (a NaN key sorts last: n)."""
    return np.searchsorted(cdf, u, side="right").astype(np.int64)


def search_device(cdf, u):
    """The contract of asmc_search (include/asmc.h): `search`, except that a NaN key gives 0 and a key below 1 never gives n."""
    cdf, u = np.asarray(cdf), np.asarray(u)
    idx = search(cdf, u)
    idx[np.isnan(u)] = 0
    idx[(u < 1.0) & (idx >= cdf.size)] = cdf.size - 1
    return idx


def guide(cdf, nb, side="right"):
    """G[b] = #{k : cdf[k] <= b / nb}, b = 0 .. nb, the keys formed as (double)b / (double)nb."""
    return np.searchsorted(cdf, np.arange(nb + 1, dtype=np.float64) / np.float64(nb), side=side).astype(np.int64)


def bucket(u, nb, settle=True):
    """The bucket b with b / nb <= u < (b + 1) / nb in the kernels' own fp64 expressions, for keys in [0, 1): the truncated
    product, then the two settling loops (without them the rule fails on keys that ARE some b / nb)."""
    u = np.asarray(u, dtype=np.float64)
    fnb = np.float64(nb)
    b = np.minimum((u * fnb).astype(np.int64), nb - 1)
    if settle:
        while True:
            down = (b > 0) & (b.astype(np.float64) / fnb > u)
            if not down.any():
                break
            b = b - down
        while True:
            up = (b < nb - 1) & ((b + 1).astype(np.float64) / fnb <= u)
            if not up.any():
                break
            b = b + up
    return b


def guided_window(cdf, u, nb, G=None, settle=True):
    """(lo, hi) of every key's search window: [G[b], G[b + 1]] for keys in [0, 1), the full range [0, n] otherwise."""
    u = np.asarray(u, dtype=np.float64)
    G = guide(cdf, nb) if G is None else G
    lo, hi = np.zeros(u.size, dtype=np.int64), np.full(u.size, len(cdf), dtype=np.int64)
    inside = (u >= 0.0) & (u < 1.0)
    b = bucket(u[inside], nb, settle)
    lo[inside], hi[inside] = G[b], G[b + 1]
    return lo, hi


def guided_search(cdf, u, nb, G=None, settle=True):
    """The bisection of k_search_guided inside its window: on a non-decreasing cdf that is the full answer clipped into the
    window, so it equals `search` exactly when the window contains the answer."""
    lo, hi = guided_window(cdf, u, nb, G, settle)
    idx = np.clip(search(cdf, u), lo, hi)
    idx[np.isnan(u)] = 0
    return idx


def keys(cdf, nbs=(), buckets=64):
    """The named key set for a cdf of length n (dict name -> array): 0.0; every b / nb and its two neighbours for `buckets`
    buckets spread over the range, for every nb given; exact hits on cdf values; the largest double below 1; 1, 2, -0.0, -1, inf
    and NaN."""
    cdf = np.asarray(cdf, dtype=np.float64)
    n = cdf.size
    out = {"zero": np.array([0.0])}
    for nb in nbs:
        b = np.unique(np.concatenate([np.linspace(0, nb, buckets).astype(np.int64), [0, 1, nb - 1, nb]]))
        b = b[(b >= 0) & (b <= nb)]
        e = b.astype(np.float64) / np.float64(nb)
        out[f"edges{nb}"] = np.concatenate([e, np.nextafter(e, 2.0), np.nextafter(e, -1.0)])
    hits = cdf[np.unique(np.linspace(0, n - 1, min(n, 97)).astype(np.int64))]
    hits = hits[np.isfinite(hits)]
    out["hits"] = np.concatenate([hits, np.nextafter(hits, -1.0), np.nextafter(hits, 2.0)])
    out["below_one"] = np.array([np.nextafter(1.0, 0.0)])
    out["outside"] = np.array([1.0, 2.0, -0.0, -1.0, np.inf])
    out["nan"] = np.array([np.nan])
    return out


def staircase_cdf(n, nb):
    """A cdf whose every value IS a bucket edge, in runs of n // nb equal values: cdf[k] = min((k // r + 1) / nb, 1), r = n // nb.
    A key one ulp below an edge then has entries of the cdf between itself and the edge: the case in which a bucket taken
    from the truncated product alone (no settling loops) opens its window above the answer."""
    r = max(n // nb, 1)
    return np.minimum((np.arange(n) // r + 1).astype(np.float64) / np.float64(nb), 1.0)


def edge_keys(nb, every=1):
    """b / nb and its two neighbours for every `every`-th bucket, inside [0, 1)."""
    e = np.arange(0, nb, every, dtype=np.float64) / np.float64(nb)
    u = np.concatenate([e, np.nextafter(e, 2.0), np.nextafter(e[1:], -1.0), [np.nextafter(1.0, 0.0)]])
    return u[(u >= 0.0) & (u < 1.0)]


def all_keys(cdf, nbs=(), buckets=64):
    return np.concatenate(list(keys(cdf, nbs, buckets).values()))


# ---- uniforms --------------------------------------------------------------------------------------------------------------------------------
def pcg64_state(rng):
    """{state_hi, state_lo, inc_hi, inc_lo} of a PCG64 Generator (the layout include/asmc.h takes)."""
    st = rng.bit_generator.state
    assert st["bit_generator"] == "PCG64"
    s, inc = st["state"]["state"], st["state"]["inc"]
    m = (1 << 64) - 1
    return np.array([s >> 64, s & m, inc >> 64, inc & m], dtype=np.uint64)


def pcg64_uniforms(rng, offset, n):
    """Doubles offset .. offset + n - 1 of the stream behind `rng` (which is left untouched)."""
    bg = np.random.PCG64()
    bg.state = rng.bit_generator.state
    bg.advance(int(offset))
    return np.random.Generator(bg).random(n)


def systematic(n_out, j0, n_total, u0=0.0, v=None):
    off = np.float64(u0) if v is None else np.asarray(v, dtype=np.float64)
    return ((np.float64(j0) + np.arange(n_out, dtype=np.float64)) + off) / np.float64(n_total)


# ---- rows ------------------------------------------------------------------------------------------------------------------------------------
def gather(idx, x, ll, lp, lq, stride=None):
    """Rows idx of (x, ll, lp, lq).  `stride` (elements between rows; default the row length) exists for the planted mistake."""
    idx = np.asarray(idx, dtype=np.int64)
    if stride is None:
        xo = x[idx]
    else:
        flat = np.ascontiguousarray(x).reshape(-1)
        d = x.shape[1]
        xo = flat[(idx[:, None] * stride + np.arange(d)[None, :]) % flat.size]
    return xo, ll[idx], lp[idx], lq[idx]


def valid_rows(ll, lp, keep_pos_inf=False):
    """Rows the compaction keeps: finite log-likelihood and log-prior (log q plays no part)."""
    ok = np.isfinite(ll) & np.isfinite(lp)
    if keep_pos_inf:  # the planted mistake: only NaN and -inf rejected
        ok = ~(np.isnan(ll) | np.isnan(lp) | (ll == -np.inf) | (lp == -np.inf))
    return ok


def compact(x, ll, lp, lq, keep_pos_inf=False):
    ok = valid_rows(ll, lp, keep_pos_inf)
    return x[ok], ll[ok], lp[ok], lq[ok]


def select_range(u, lo, hi):
    u = np.asarray(u)
    return u[(u >= lo) & (u < hi)]


def colsum(rows):
    """(column sums of the rows in long double, sum of |entries| per column): the latter scales the moments tolerance."""
    r = np.asarray(rows, dtype=LD)
    return r.sum(axis=0), np.abs(r).sum(axis=0)


def bits_equal(a, b):
    """Bit for bit, NaN payloads and signed zeros included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- the reference's weights (for the golden indices) -----------------------------------------------------------------------------------
def normalized_weights(ll, lp, lq, beta0, beta):
    """w = exp(log_w - logsumexp(log_w)), log_w = lw + (logsumexp(lw) - log N), lw = (beta0 - beta) lq + (beta - beta0) (ll + lp):
    the reference's fp64 expressions (its resampling weights; an ulp here moves an index with probability ~ N u per draw)."""
    ll, lp, lq = (np.asarray(a, dtype=np.float64) for a in (ll, lp, lq))
    lw = (np.float64(beta0) - np.float64(beta)) * lq + (np.float64(beta) - np.float64(beta0)) * (ll + lp)

    def lse(a):
        m = a.max()
        return m + math.log(np.exp(a - m).sum())
    log_w = lw + (lse(lw) - math.log(lw.size))
    return np.exp(log_w - lse(log_w))


def resample_indices(ll, lp, lq, beta0, beta, u):
    w = normalized_weights(ll, lp, lq, beta0, beta)
    return search(exact_cdf(w, normalize=True), u)
