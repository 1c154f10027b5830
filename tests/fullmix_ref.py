"""Long-double restatement of GaussianMixture's value and gradient, its tolerance formulas, and the input generators the tests share.

The restatement's inputs are the tables exactly as the class hands them to the device (`tables(target)`): the factorisation
error of the constructor is not part of the kernel's contract.

Tolerances (u = 2^-53; none comes from a device result).  With r = fl(x - mu_c), a_c = |W_c| |r| (entrywise absolute values):

  value.  v_i = sum_j W_ij r_j is a chain of at most d fused multiply-adds per lane, four partial chains added in two steps:
    |dv_i| <= (d/4 + 3) u a_i <= (d + 2) u a_i, r's own rounding included.  q = sum v_i^2 in the order of i adds d u q, so
    |dq| <= (2 (d + 2) + d + 1) u sum a_i^2 = (3 d + 5) u sum a_i^2, and term_c = logw_c - q / 2 carries
    (3 d + 5) u / 2 sum a^2 + u |term_c| <= (3 d + 8) u (|logw_c| + sum a^2 / 2).  The largest term dominates the log-sum-exp,
    whose own error (C > 1 only: at most C rescalings of the running sum, one exp and one add each, one log, all within an ulp
    or two, on a sum in [1, C]) is at most (3 C + 4) u absolute, plus the rounding of the result:
        tol_value = (3 d + 8) u max_c(|logw_c| + sum_i a_ci^2 / 2) + [C > 1] (3 C + 4) u + 4 ulp(value).
  gradient entry j.  W^T v is again a chain of at most d fused multiply-adds on v (error (d + 2) u a each) times the
    responsibility, whose relative error is the absolute error of term_c - value, at most 2 tol_value:  with
    m_j = sum_c resp_c (|W_c|^T a_c)_j
        tol_grad_j = (2 d + 8) u m_j + 2 tol_value m_j + 4 ulp(G_j) + 4 * 2^-1074 sum_c (|W_c|^T a_c)_j.
    The last term is gradual underflow: a responsibility below 2^-1022 is a subnormal with an absolute, not a relative,
    rounding error of up to 2^-1074 (a flat component next to far Gaussian ones leaves nothing else in the gradient).

numpy's own fp64 evaluation sits at 0.16 (value) and 0.07 (gradient) of these over the grid of tests/test_fullmix_ref.py.
"""
import numpy as np

LD = np.longdouble
U = 2.0**-53


def tables(target):
    """(logw [C], mu [C, d], whiten [C, d, d], lower [d] | None, upper [d] | None): fp64, as uploaded."""
    return (np.asarray(target.logw, dtype=np.float64), np.asarray(target.mu, dtype=np.float64),
            np.asarray(target.whiten, dtype=np.float64), target.lower, target.upper)


# ---- generators ---------------------------------------------------------------------------------------------------------
def make_target(d, C, cond, seed, kind="plain", bounds=False):
    """A mixture of C components in d dimensions whose precisions have condition number `cond` (eigenvalues spread
    geometrically over [cond^-1/2, cond^1/2], random eigenvectors).  kind: "plain" (normalised, from covariances), "flat"
    (component 0 has a zero precision), "singular" (component 0's smallest eigenvalue is zero).  Returns (target, meta); meta
    holds the covariances / precisions the target was made from (the mutations of the reference test use them)."""
    from aspire_amd import GaussianMixture

    g = np.random.default_rng([seed, d, C, int(np.log10(cond))])
    mu = 1.5 * g.normal(size=(C, d))
    lam = np.geomspace(cond**-0.5, cond**0.5, d) if d > 1 else np.ones(1)
    cov, prec = np.zeros((C, d, d)), np.zeros((C, d, d))
    for c in range(C):
        Q = np.linalg.qr(g.normal(size=(d, d)))[0]
        lc = lam.copy()
        if c == 0 and kind == "flat":
            lc[:] = 0.0
        if c == 0 and kind == "singular":
            lc[0] = 0.0
        prec[c] = (Q * lc) @ Q.T
        prec[c] = 0.5 * (prec[c] + prec[c].T)
        if kind == "plain":
            cov[c] = (Q / lc) @ Q.T
            cov[c] = 0.5 * (cov[c] + cov[c].T)
    w = g.uniform(0.5, 1.5, size=C)
    b = (-9.0, np.linspace(8.5, 9.5, d)) if bounds else None  # a few rows in a hundred fall outside
    if kind == "plain":
        t = GaussianMixture(mu, cov, weights=w, bounds=b)
    else:
        t = GaussianMixture(mu, precisions=prec, weights=w, bounds=b, normalized=False)
    return t, dict(cov=cov, prec=prec, lam=lam, kind=kind)


def make_rows(target, n, seed, dtype=np.float64):
    """n rows drawn around the components' means at the scale of the widest finite axis of each (so the quadratic forms are of
    order d at condition 1 and spread over many orders at 1e6), as `dtype`."""
    g = np.random.default_rng([seed, n, target.dims])
    c = g.integers(0, target.n_components, size=n)
    z = g.normal(size=(n, target.dims))
    scale = np.ones(target.n_components)
    for k in range(target.n_components):
        dg = np.abs(np.diag(target.whiten[k]))
        scale[k] = 1.0 / dg[dg > 0].min() if np.any(dg > 0) else 1.0
    x = target.mu[c] + z * np.minimum(scale[c], 2.0)[:, None]
    return np.ascontiguousarray(x.astype(dtype))


def special_rows(target, dtype=np.float64):
    """Rows of the non-finite contract and the edges of the box: NaN (also together with an inf and with a coordinate outside
    the box), +inf, -inf, on / just inside / just outside each end of each bound, and rows too far for fp64."""
    d = target.dims
    base = np.asarray(target.mu[0], dtype=np.float64).copy()
    if target.lower is not None:
        base = np.clip(base, target.lower + 0.25, target.upper - 0.25)
    rows = []

    def put(j, v, j2=None, v2=None):
        r = base.copy()
        r[j] = v
        if j2 is not None:
            r[j2] = v2
        rows.append(r)

    for j in sorted({0, d // 2, d - 1}):
        put(j, np.nan)
        put(j, np.inf)
        put(j, -np.inf)
        put(j, np.nan, (j + 1) % d, np.inf)
        put(j, 1e200)
        put(j, -1e200)
        if target.lower is not None:
            lo, hi = dtype(target.lower[j]), dtype(target.upper[j])
            for end, inward in ((lo, dtype(np.inf)), (hi, dtype(-np.inf))):
                put(j, end)
                put(j, np.nextafter(end, inward))
                put(j, np.nextafter(end, -inward))
            put(j, np.nan, (j + 1) % d, target.upper[(j + 1) % d] + 1.0)
    rows.append(np.full(d, 1e200))
    rows.append(base)
    with np.errstate(over="ignore"):  # (1e200 as fp32 is +inf: one more row of that kind)
        x = np.asarray(rows).astype(dtype)
    return np.ascontiguousarray(x)


DIMS = (1, 2, 3, 4, 8, 16, 31, 32, 33, 48, 64, 65, 100, 128)
COMPONENTS = (1, 2, 4, 5, 8)
KINDS = ("plain", "flat", "singular")


def grid():
    """The shared case list: (d, C, cond, kind, bounds, dtype, n).  Every d meets every C, both condition numbers, both row
    types, bounds on and off and the three kinds, in a rotation (not the full product: each case costs a long-double
    reference); n is 257 for narrow rows and 65 for wide ones, so a case stays within a second on the host."""
    cases = []
    for i, d in enumerate(DIMS):
        for k, C in enumerate(COMPONENTS):
            t = i + k
            cond = (1.0, 1e6)[t % 2]
            kind = KINDS[(i + 2 * k) % 3] if d > 1 else ("plain", "flat")[k % 2]
            bounds = bool((t // 2) % 2)
            dtype = (np.float64, np.float32)[(i + k // 2) % 2]
            cases.append((d, C, cond, kind, bounds, dtype, 257 if d <= 32 else 65))
    return cases


# ---- the restatement ------------------------------------------------------------------------------------------------------
def _classes(x, lower, upper):
    nan_row = np.isnan(x).any(axis=1)
    bad = np.isinf(x).any(axis=1)
    if lower is not None:
        with np.errstate(invalid="ignore"):
            bad = bad | ((x < lower) | (x > upper)).any(axis=1)
    return nan_row, bad & ~nan_row


def reference(target, x):
    """dict(value [n] fp64, grad [n, d] fp64, tol_value [n], tol_grad [n, d]) from long-double arithmetic on the fp64 tables
    and the rows exactly as given (fp32 rows are exact in long double)."""
    logw, mu, W, lower, upper = tables(target)
    C, d = mu.shape
    x64 = np.asarray(x, dtype=np.float64)
    n = x64.shape[0]
    nan_row, bad = _classes(x64, lower, upper)
    plain = ~(nan_row | bad)
    xs = np.where(plain[:, None], x64, 0.0)
    terms = np.zeros((n, C), dtype=LD)
    tv = np.zeros((n, C, d), dtype=LD)  # W^T v
    h = np.zeros((n, C))
    mabs = np.zeros((n, C, d))
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(C):
            r = xs.astype(LD) - mu[c].astype(LD)
            Wc = W[c].astype(LD)
            v = r @ Wc.T
            terms[:, c] = LD(logw[c]) - LD(0.5) * (v * v).sum(axis=1)
            tv[:, c] = v @ Wc
            r64 = np.abs(xs - mu[c])
            a = r64 @ np.abs(W[c]).T
            h[:, c] = abs(logw[c]) + 0.5 * (a * a).sum(axis=1)
            mabs[:, c] = a @ np.abs(W[c])
        m = terms.max(axis=1)
        value_ld = m + np.log(np.exp(terms - m[:, None]).sum(axis=1)) if C > 1 else terms[:, 0]
        resp = np.exp(terms - value_ld[:, None])
        grad_ld = -(resp[:, :, None] * tv).sum(axis=1)
        value = value_ld.astype(np.float64)
        value = np.where(bad, -np.inf, value)
        value = np.where(nan_row, np.nan, value)
        fin = np.isfinite(value)
        grad = np.where(fin[:, None], grad_ld.astype(np.float64), 0.0)
        resp64 = np.where(fin[:, None], resp.astype(np.float64), 0.0)
        tol_value = (3 * d + 8) * U * h.max(axis=1) + (C > 1) * (3 * C + 4) * U + 4 * np.spacing(np.abs(np.where(fin, value, 0.0)))
        mj = (resp64[:, :, None] * mabs).sum(axis=1)
        tol_grad = ((2 * d + 8) * U * mj + 2 * tol_value[:, None] * mj + 4 * np.spacing(np.abs(grad))
                    + 4 * 2.0**-1074 * mabs.sum(axis=1))
    return dict(value=value, grad=grad, tol_value=tol_value, tol_grad=tol_grad)


def compare(ref, value, grad=None):
    """(worst value error, worst gradient error) in units of the tolerances over every finite element; inf when the non-finite
    pattern differs from the restatement's (NaN where NaN, -inf where -inf, nothing else non-finite) or a gradient row of a
    non-finite value is not exactly zero."""
    value = np.asarray(value, dtype=np.float64)
    fin = np.isfinite(ref["value"])
    ok = (np.array_equal(np.isnan(value), np.isnan(ref["value"])) and np.array_equal(np.isneginf(value), np.isneginf(ref["value"]))
          and not np.isposinf(value).any())
    if not ok or value.shape != ref["value"].shape:
        return np.inf, np.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        wv = float(np.max(np.abs(value[fin] - ref["value"][fin]) / ref["tol_value"][fin], initial=0.0))
    if grad is None:
        return wv, 0.0
    grad = np.asarray(grad, dtype=np.float64)
    if grad.shape != ref["grad"].shape or not np.all(np.isfinite(grad)) or np.any(grad[~fin] != 0.0):
        return wv, np.inf
    err = np.abs(grad[fin] - ref["grad"][fin])
    tol = ref["tol_grad"][fin]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / tol)
    return wv, float(np.max(ratio, initial=0.0))


# ---- numpy's own fp64 evaluation, and its mutations ---------------------------------------------------------------------
MUTATIONS = ("dropped_row", "transposed_factor", "missing_weight", "swapped_bound", "no_responsibilities", "rPr")


def numpy_fp64(target, x, mutate=None, meta=None):
    """(value, grad) by plain fp64 numpy on the same tables; `mutate` plants one of MUTATIONS."""
    logw, mu, W, lower, upper = tables(target)
    C, d = mu.shape
    x = np.asarray(x, dtype=np.float64)
    if mutate == "swapped_bound" and lower is not None:
        lower, upper = upper, lower
    if mutate == "transposed_factor":
        W = np.ascontiguousarray(W.transpose(0, 2, 1))
    if mutate == "missing_weight":
        logw = np.zeros_like(logw)
    nan_row, bad = _classes(x, lower, upper)
    plain = ~(nan_row | bad)
    xs = np.where(plain[:, None], x, 0.0)
    terms = np.zeros((x.shape[0], C))
    tv = np.zeros((x.shape[0], C, d))
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(C):
            r = xs - mu[c]
            v = r @ W[c].T
            q = (v * v).sum(axis=1)
            if mutate == "rPr":  # the precision itself, as the inverse of the covariance the target was made from
                P = np.linalg.inv(meta["cov"][c])
                q = ((r @ P) * r).sum(axis=1)
            q = np.where(np.isnan(q), np.inf, q)
            terms[:, c] = logw[c] - 0.5 * q
            tv[:, c] = v @ W[c]
        m = terms.max(axis=1)
        value = m + np.log(np.exp(terms - m[:, None]).sum(axis=1)) if C > 1 else terms[:, 0].copy()
        value = np.where(np.isneginf(m), -np.inf, value)
        resp = np.exp(terms - value[:, None])
        if mutate == "no_responsibilities":
            resp = np.ones_like(resp)
        value = np.where(bad, -np.inf, value)
        value = np.where(nan_row, np.nan, value)
        grad = np.where(np.isfinite(value)[:, None], -(resp[:, :, None] * tv).sum(axis=1), 0.0)
    if mutate == "dropped_row" and len(value) > 1:
        k = len(value) // 2
        value = np.concatenate([value[:k], value[k + 1:], value[-1:]])
        grad = np.concatenate([grad[:k], grad[k + 1:], grad[-1:]])
    return value, grad
