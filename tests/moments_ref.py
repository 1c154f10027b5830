"""Host restatement, in numpy long double (80-bit), of the population moments (asmc_colsum, asmc_centered_gram, asmc_mean_gram), the
device-side reference fit (asmc_reference_factor), and the built-in densities (asmc_mixture_logpdf, asmc_mixture_logpdf_premap, the
log q of asmc_gaussian_draw), with the magnitudes their tolerances are made of, the tolerance formulas themselves
and the input generators - shared by tests/test_moments_ref.py (CPU: the formulas can be met and have teeth) and
tests/test_gpu_moments_density.py (the kernels).

fp32 storage: every function takes the fp32-rounded inputs widened to fp64 (exact); the outputs of the kernels are fp64 sums, so fp32
rows earn no extra tolerance.
"""
import numpy as np
from scipy.linalg import solve_triangular

from transform_ref import LD, gap_ulps, same_nonfinite, ulp64  # noqa: F401  (re-exported)

U = 2.0**-53  # unit roundoff of fp64
assert np.finfo(LD).nmant >= 63, "the restatement needs an extended long double"
LOG_2PI = np.log(LD(2) * np.arccos(LD(-1)))


# ---- restatements -------------------------------------------------------------------------------------------------------------------
def colsum(x):
    """(sum_i x_ij in long double, sum_i |x_ij|)."""
    x = np.asarray(x, dtype=np.float64)
    return x.astype(LD).sum(0), np.abs(x).sum(0)


def centered_gram(x, c):
    """(sum_i a_i a_i^T in long double, sum_i |a_ij| |a_ik|, sum_i |a_ij|) with a = fl(x - c), the fp64 difference every kernel forms
    first: what remains is the error of n products and their sum, in any order.
    The sum itself: a is cut into four slices of 20 bits below its largest exponent (a = h_0 + h_1 + h_2 + h_3 + a rest below 2^-83 of
    the largest entry), each slice an integer multiple of its quantum, so that over 4096 rows every product sum H_p^T H_q is an
    integer below 2^52 - exact in fp64, whatever the order a BLAS takes; the exact pieces are added up in long double.  (numpy's own
    long-double matrix product agrees to its own rounding, n 2^-64 of the magnitudes, and takes 20 ns per product.)"""
    x, c = np.asarray(x, dtype=np.float64), np.asarray(c, dtype=np.float64)
    d = x.shape[1]
    g, mag, s1 = np.zeros((d, d), dtype=LD), np.zeros((d, d)), np.zeros(d)
    a_all = x - c
    top = float(np.abs(a_all).max()) if a_all.size else 0.0
    e = int(np.frexp(top)[1]) if top > 0 else 0  # |a| < 2^e
    for i in range(0, len(x), 4096):
        a = a_all[i:i + 4096]
        mag += np.abs(a).T @ np.abs(a)
        s1 += np.abs(a).sum(0)
        sl, r = [], a
        for p in range(4):
            k = e - 20 - 21 * p  # the slice's quantum 2^k: |r| <= 2^(k + 20)
            h = np.rint(np.ldexp(r, -k))  # integers of at most 2^20
            sl.append((h, k))
            r = r - np.ldexp(h, k)  # exact
        for p, (hp, kp) in enumerate(sl):
            for q, (hq, kq) in enumerate(sl):
                if p <= q:
                    m = np.ldexp((hp.T @ hq).astype(LD), kp + kq)
                    g += m if p == q else m + m.T
    return g, mag, s1


def premap_t(x, premap):
    """t = clip(a x + b, lo, hi) in the kernels' own fp64 arithmetic (one product, one sum), NaN passing through (numpy's clip)."""
    a, b, lo, hi, _ = premap
    with np.errstate(all="ignore"):
        v = np.asarray(x, dtype=np.float64) * a + b
        return np.where(v < lo, lo, np.where(v > hi, hi, v))


def mixture_logpdf(x, logw, mu, prec, premap=None, chunk=8192):
    """(log sum_c exp(logw_c - q_c / 2) [+ sum_j h_j t_j^2] per row in long double, max_c (|logw_c| + q_c / 2) [+ sum_j |h_j| t_j^2],
    the premap's sensitivity sum_j ulp(a x + b) (2 |t - mu| prec + 2 |h t|) maximised over the components, 0 without a premap).
    q_c = sum_j (t_j - mu_cj)^2 prec_cj at t = x or premap_t(x).  Non-finite rule: one component - the term itself;
    several - every term -inf or NaN (the maximum that ignores NaN is -inf): the sum of the terms, -inf or NaN; so a NaN coordinate
    gives NaN for every C, and far rows or components of weight zero give -inf."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    logw, mu, prec = np.atleast_1d(np.asarray(logw, dtype=np.float64)), np.atleast_2d(mu), np.atleast_2d(prec)
    C = len(logw)
    out, mag, sens = np.empty(len(x), dtype=LD), np.empty(len(x)), np.zeros(len(x))
    with np.errstate(all="ignore"):
        for i in range(0, len(x), chunk):
            xs = x[i:i + chunk]
            t64 = xs if premap is None else premap_t(xs, premap)
            t = t64.astype(LD)
            terms = np.empty((C, len(xs)), dtype=LD)
            sn, m = np.zeros(len(xs)), np.zeros(len(xs))
            for c in range(C):
                dlt = t - mu[c].astype(LD)
                hq = LD(0.5) * (dlt * dlt * prec[c].astype(LD)).sum(1)
                terms[c] = LD(logw[c]) - hq
                m = np.fmax(m, (abs(logw[c]) if np.isfinite(logw[c]) else 0.0) + hq.astype(np.float64))
                if premap is not None:
                    a, b, lo, hi, h = premap
                    v = xs * a + b
                    free = (v >= lo) & (v <= hi)  # (a clamped coordinate does not move with a x + b)
                    s = np.where(free, ulp64(v) * (2 * np.abs(t64 - mu[c]) * prec[c] + 2 * np.abs(h * t64)), 0.0)
                    sn = np.fmax(sn, np.where(np.isfinite(s), s, 0.0).sum(1))
            if C == 1:
                r = terms[0].copy()
            else:
                best = np.fmax.reduce(terms, axis=0)
                cold = ~(best > -np.inf)
                safe = np.where(cold, LD(0), best)
                r = np.where(cold, terms.sum(0), safe + np.log(np.exp(terms - safe).sum(0)))
            if premap is not None:
                h = np.asarray(premap[4], dtype=np.float64).astype(LD)
                r = r + (h * t * t).sum(1)
                m = m + (np.abs(premap[4]) * t64 * t64).sum(1)
            out[i:i + chunk], mag[i:i + chunk], sens[i:i + chunk] = r, m, sn
    return out, mag, sens


def gaussian_logq(x, mu, sigma):
    """(log N(x; mu, diag sigma^2) per row in long double, q / 2 + sum |log sigma| + d log(2 pi) / 2)."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64)).astype(LD)
    mu, sigma = np.asarray(mu, dtype=np.float64).astype(LD), np.asarray(sigma, dtype=np.float64).astype(LD)
    z = (x - mu) / sigma
    half_q, ls, cst = LD(0.5) * (z * z).sum(1), np.log(sigma), LD(0.5) * x.shape[1] * LOG_2PI
    return -half_q - ls.sum() - cst, (half_q + np.abs(ls).sum() + cst).astype(np.float64)


def cholesky_ld(a):
    """Plain long-double Cholesky loop; None when a pivot is not a positive finite number."""
    a = np.array(a, dtype=LD)
    d = len(a)
    L = np.zeros((d, d), dtype=LD)
    with np.errstate(all="ignore"):
        for j in range(d):
            p = a[j, j] - (L[j, :j] * L[j, :j]).sum()
            if not (p > 0 and p < np.inf):
                return None
            L[j, j] = np.sqrt(p)
            if j + 1 < d:
                L[j + 1:, j] = (a[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def lower_inverse_ld(L):
    """L^-1 by forward substitution, column by column, in long double."""
    d = len(L)
    X = np.zeros((d, d), dtype=LD)
    for i in range(d):
        X[i, i] = LD(1) / L[i, i]
        if i:
            X[i, :i] = -(L[i, :i] @ X[:i, :i]) / L[i, i]
    return X


def fit_gaps(cov_ld):
    """(E_L, E_Linv): the gaps, in fp64 ulps of the long-double values, between numpy / scipy in fp64 and the long-double run on the
    same covariance - the measure of its conditioning that the 8 E + 4 rule scales with."""
    c64 = np.asarray(cov_ld).astype(np.float64)
    L64 = np.linalg.cholesky(c64)
    Li64 = solve_triangular(L64, np.eye(len(c64)), lower=True)
    L = cholesky_ld(cov_ld)
    Li = lower_inverse_ld(L)
    low = np.tril(np.ones(c64.shape, dtype=bool))
    return gap_ulps(L64[low], L[low]), gap_ulps(Li64[low], Li[low])


JITTERS = [0.0] + [1e-12 * 100.0**k for k in range(11)]  # twelve tries: 0, 1e-12, then x 100


def covariance(gram, n_cov):
    """The symmetrised G / max(n_cov - 1, 1), in long double."""
    g = np.asarray(gram, dtype=np.float64).astype(LD)
    with np.errstate(all="ignore"):
        return LD(0.5) * (g + g.T) / LD(max(n_cov - 1, 1))


def jitter_scale(cov):
    with np.errstate(all="ignore"):
        t = np.trace(cov) / LD(len(cov))
    return t if (t > 0 and t < np.inf) else LD(1)


def reference_fit(sums, gram, n_mean, n_cov):
    """(mu, L, Linv, tries, the covariance that was factored - jitter included) of asmc_reference_factor: mu = sum / n_mean; cov as
    `covariance`; L = chol(cov + jitter scale I) at the first of the twelve jitters that factors, scale = mean(diag cov) when that is
    positive and finite, else 1; Linv by forward substitution.  tries = the index of that jitter; -1, L = Linv = None: none did."""
    mu = np.asarray(sums, dtype=np.float64).astype(LD) / LD(n_mean)
    cov = covariance(gram, n_cov)
    scale = jitter_scale(cov)
    for tries, jit in enumerate(JITTERS):
        a = cov + LD(jit) * scale * np.eye(len(cov), dtype=LD)
        L = cholesky_ld(a)
        if L is not None:
            return mu, L, lower_inverse_ld(L), tries, a
    return mu, None, None, -1, None


# ---- tolerances (none is taken from an implementation's output) ----------------------------------------------------------------------
def tol_colsum(n, sum_abs):
    """n u sum_i |x_ij|: the bound of a sum of n numbers in any order."""
    return n * U * np.asarray(sum_abs)


def tol_gram(n, mag):
    """(n + 4) u sum_i |a_ij| |a_ik|: n products, summed in any order, a few roundings of the reductions behind the kernels."""
    return (n + 4) * U * np.asarray(mag)


def tol_mean_gram(n, n_mean, mag, s1, sum_abs):
    """tol_gram plus the exact effect of a centre that is off by at most delta_j = tol_colsum_j / n_mean:
    sum (a_j - e_j)(a_k - e_k) - sum a_j a_k = -e_j sum a_k - e_k sum a_j + n e_j e_k."""
    dl = tol_colsum(n, sum_abs) / n_mean
    return tol_gram(n, mag) + dl[:, None] * s1[None, :] + dl[None, :] * s1[:, None] + n * dl[:, None] * dl[None, :]


def tol_mixture(d, mag, ref, sens=0.0):
    """(d + 8) u max_c (|logw_c| + q_c / 2) + 4 ulp of the result (+ the premap's sensitivity), per row."""
    with np.errstate(all="ignore"):
        r = np.asarray(ref, dtype=np.float64)
        return (d + 8) * U * np.asarray(mag) + 4 * np.where(np.isfinite(r), ulp64(np.where(np.isfinite(r), r, 0.0)), 0.0) + sens


def half_ulp32(ref):
    """Half the fp32 spacing at the fp64 magnitude of ref (one rounding of an fp64-accurate value to fp32 storage)."""
    a = np.abs(np.asarray(ref, dtype=np.float64))
    e = np.frexp(np.where(a > 0, a, 1.0))[1] - 1
    return np.where(a > 0, np.ldexp(1.0, np.maximum(e, -126) - 24), np.ldexp(1.0, -150))


def worst(err, tol):
    """The largest error in units of its tolerance."""
    err, tol = np.asarray(err, dtype=np.float64), np.broadcast_to(np.asarray(tol, dtype=np.float64), np.shape(err))
    if err.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        return float(np.max(np.where(err == 0, 0.0, err / tol)))


def compare(got, ref, tol, what, quiet=False):
    """The whole comparison of one result: the same non-finite pattern, every finite element within its tolerance; prints the
    tolerance and the worst error in units of it, returns that ratio."""
    got, refd = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=LD)
    assert got.shape == refd.shape, (what, got.shape, refd.shape)
    assert same_nonfinite(got, refd.astype(np.float64)), (what, "non-finite pattern")
    fin = np.isfinite(refd)
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), got.shape)
    with np.errstate(all="ignore"):
        err = np.abs(got.astype(LD) - refd).astype(np.float64)
    w = worst(err[fin], tol[fin])
    if not quiet:
        print(f"TOL {what}: max tolerance {float(np.max(tol[fin])) if fin.any() else 0.0:.3g}, worst error {w:.3g} of its tolerance"
              f" ({int(fin.sum())} finite, {int((~fin).sum())} non-finite elements)")
    assert w <= 1.0, (what, w)
    return w


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def rounded(x, f32):
    """x as the device stores it, widened back to fp64."""
    return np.asarray(x, dtype=np.float32).astype(np.float64) if f32 else np.asarray(x, dtype=np.float64)


def away_from_zero(z):
    """|.| >= 0.5: a dropped or doubled element is then far outside every tolerance."""
    return np.where(z < 0, z - 0.5, z + 0.5)


def population(n, d, kind="bulk", seed=0, f32=False):
    """[n, d] rows: 'bulk' - columns of scale 1..3 and |x| >= 0.5; 'offset' - 1e6 + N(0, 1) with |.| >= 0.5, the spread a millionth of
    the offset, where only a truly centred kernel keeps any digit."""
    g = np.random.default_rng([seed, n, d])
    z = away_from_zero(g.normal(size=(n, d)))
    x = 1e6 + z if kind == "offset" else z * np.linspace(1.0, 3.0, d)
    return rounded(x, f32)


def centre(x):
    """A host-supplied centre: numpy's fp64 column mean."""
    return x.sum(0) / len(x)


def mixture_params(d, C, seed=0, zero_weight=None):
    """(logw, mu, prec) of a normalised diagonal mixture with unequal weights; zero_weight: 'one' - component 1 (0 when C = 1) has
    logw = -inf, 'all' - every component."""
    g = np.random.default_rng([seed, d, C, 7])
    mu, var = g.normal(size=(C, d)), g.uniform(0.5, 2.0, size=(C, d))
    w = g.uniform(0.5, 1.5, size=C)
    logw = np.log(w / w.sum()) - 0.5 * d * np.log(2 * np.pi) - 0.5 * np.log(var).sum(1)
    if zero_weight == "one":
        logw[min(1, C - 1)] = -np.inf
    elif zero_weight == "all":
        logw[:] = -np.inf
    return logw, mu, 1.0 / var


EDGE_ROWS = 14  # mixture_rows needs n > EDGE_ROWS + 3 to hold them all; a smaller n takes the ones that fit


def mixture_rows(n, d, mu, prec, seed=0, f32=False, premap=None):
    """[n, d] rows 2 N(0, 1) with |.| >= 0.5 and, from row 2 on while they fit, the edge rows: 1e4 sigma away on either side (every exp
    underflows, the result stays finite), +inf and -inf in one coordinate, NaN in the first, a middle and the last coordinate with
    clean rows between them (a NaN must not cross the flat kernel's butterfly), with a premap a NaN in a bounded and in an unbounded
    coordinate and rows exactly on and just beyond both clamp ends; the last row but one is clean between two NaN rows (the ragged
    tile).  Returns (x, the indices of the rows with a NaN)."""
    g = np.random.default_rng([seed, n, d, 11])
    x = 2.0 * away_from_zero(g.normal(size=(n, d)))
    sig = 1.0 / np.sqrt(prec[0])
    mid, last = d // 2, d - 1
    edges = [mu[0] + 1e4 * sig, mu[0] - 1e4 * sig]
    nan_at = []

    def poke(j, v, base=None):
        r = (x[min(len(edges) + 2, n - 1)] if base is None else base).copy()
        r[j] = v
        edges.append(r)
        if np.isnan(v):
            nan_at.append(len(edges) - 1)

    poke(0, np.inf), poke(last, -np.inf), poke(0, np.nan)
    edges.append(x[min(1, n - 1)].copy())
    poke(mid, np.nan)
    edges.append(x[0].copy())
    poke(last, np.nan)
    if premap is not None:
        a, b, lo, hi, _ = premap
        bounded = np.flatnonzero(np.isfinite(lo))
        free = np.flatnonzero(~np.isfinite(lo))
        with np.errstate(all="ignore"):
            on_lo, on_hi = np.where(np.isfinite(lo), (lo - b) / a, -3.0), np.where(np.isfinite(hi), (hi - b) / a, 3.0)
        edges += [on_lo, on_hi, on_lo - 0.125, on_hi + 0.125]
        poke(bounded[-1], np.nan)
        if len(free):
            poke(free[0], np.nan)
    edges = edges[:max(0, min(len(edges), n - 2))]
    for k, r in enumerate(edges):
        x[2 + k] = r
    nan_rows = [2 + k for k in nan_at if k < len(edges)]
    if n >= 3 + 2 + len(edges):
        x[n - 3, 0] = x[n - 1, last] = np.nan
        nan_rows += [n - 3, n - 1]
    return rounded(x, f32), np.array(sorted(nan_rows), dtype=int)


def premap_table(d, seed=0, zero_h=False):
    """(a, b, lo, hi, h): every fourth coordinate unbounded (lo = -inf, hi = +inf), the others clamped to [-1.5, 2.25]; a, b dyadic so
    that rows can sit exactly on a clamp end in fp32 and fp64; h of both signs, or zero."""
    g = np.random.default_rng([seed, d, 13])
    a = g.choice([0.5, 1.0, 2.0], size=d)
    b = g.choice([-0.25, 0.0, 0.75], size=d)
    free = np.arange(d) % 4 == 0
    lo, hi = np.where(free, -np.inf, -1.5), np.where(free, np.inf, 2.25)
    h = np.zeros(d) if zero_h else g.choice([-0.0625, 0.0, 0.03125, 0.125], size=d)
    return a, b, lo, hi, h


FIT_DIMS = [1, 4, 20, 32, 33, 64, 100, 128]
N_MEAN, N_COV = 5003, 4097  # n_cov - 1 a power of two: the covariance of a symmetric G is exact in fp64 - the kernel's input is ours


def spd_with_condition(d, cond, seed=0):
    """Q diag(lambda) Q^T, Q a random orthogonal factor, lambda log-spaced from 1 down to 1 / cond; symmetric bit for bit."""
    g = np.random.default_rng([seed, d, 17])
    q, _ = np.linalg.qr(g.normal(size=(d, d)))
    lam = np.logspace(0, -np.log10(cond), d) if d > 1 else np.ones(1)
    a = (q * lam) @ q.T
    return 0.5 * (a + a.T)


def with_eigenvalues(d, lam, seed=0):
    """Q diag(lam) Q^T with a random orthogonal Q; symmetric bit for bit."""
    g = np.random.default_rng([seed, d, 19])
    q, _ = np.linalg.qr(g.normal(size=(d, d)))
    a = (q * np.asarray(lam, dtype=np.float64)) @ q.T
    return 0.5 * (a + a.T)


def with_lowest_eigenvalue(d, lowest, seed=0, relative=True):
    """A symmetric matrix whose other eigenvalues lie in [0.5, 2] and whose lowest is `lowest` x its own mean(diag) (relative) or
    `lowest` itself."""
    g = np.random.default_rng([seed, d, 23])
    lam = g.uniform(0.5, 2.0, size=d)
    # relative: lam_0 = lowest (lam_0 + sum of the others) / d
    lam[0] = lowest * lam[1:].sum() / (d - lowest) if relative else lowest
    return with_eigenvalues(d, lam, seed)


def all_negative(d, lowest=-3e-7, seed=0):
    """Every eigenvalue in [lowest, lowest / 3], the lowest one included: mean(diag) < 0, so the jitter's scale is 1."""
    g = np.random.default_rng([seed, d, 29])
    lam = g.uniform(lowest, lowest / 3, size=d)
    lam[0] = lowest
    return with_eigenvalues(d, lam, seed)
