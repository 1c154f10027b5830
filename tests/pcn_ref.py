"""Host restatement of the pCN / tpCN mutation step (include/asmc.h asmc_pcn_mutate / asmc_pcn_propose / asmc_pcn_accept,
DESIGN.md §3.6, csrc/asmc_pcn_dev.h), vectorised numpy written for any numpy float type: the `np.float64` run is what the device
kernels are compared with, the `np.longdouble` run of the same code measures the float64 run's own rounding error - the unit
of every tolerance of tests/test_gpu_pcn.py.

Philox, the fp64 normals and the accept uniforms come from stretch_ref / hmc_ref; the hardware-fp32 noise mode takes its draws
from the oracle's restatement (oracle.pcn_noise(..., "f32"), oracle.gamma_unit(..., "f32")).  A test helper: the product never
imports it.
"""
from __future__ import annotations

import numpy as np

import hmc_ref as H
import stretch_ref as S

TAG_GAMMA = 0x80000000
EPS64 = 2.0**-52
EPS32 = 2.0**-23
SESSION_DIMS = (4, 8, 16, 32)  # the widths asmc_pcn_ysplit_begin accepts (pcn_reg_supported): every other one returns UNSUPPORTED
BUGS = ("corr_sign", "q1_padded", "a_no_root", "shape_padded", "u_tile_local", "ragged_last_lane", "no_guard")


def pad_dim(d):
    """The width asmc_pcn_mutate zero-pads a d-dimensional problem to (its own width for 4, 8, 16, 32, 64, 128)."""
    for D in (4, 8, 16, 32, 64, 128):
        if d <= D:
            return D
    return d


# ---- draws ---------------------------------------------------------------------------------------------------------------------
def noise(seed, gid0, n, step, d, mode="f64"):
    """(xi [n, d], accept uniforms [n]) of particles gid0 .. gid0 + n - 1 at Markov step `step`."""
    u = H.accept_uniforms(seed, gid0, n, step)
    if mode == "f64":
        return H.normals(seed, gid0, n, step, d), u
    import oracle as O

    m64 = (1 << 64) - 1
    xi = np.stack([O.pcn_noise(seed, (gid0 + i) & m64, step, d, "f32")[0] for i in range(n)])
    return xi, u


def gamma_unit(shape, seed, gid0, n, step, mode="f64"):
    """Unit-scale Gamma(shape >= 1) variates, Marsaglia & Tsang (2000), as asmc_pcn_dev.h gamma_unit draws them: attempt a < 8
    takes ONE Philox block (slot 0x80000000 | a): the normal is the first of the Box-Muller pair of words 0, 1, the uniform the
    53 bits of words 2, 3; v = (1 + c z)^3, accepted when log u < z^2/2 + dd - dd v + dd log v; after 8 failures dd."""
    if mode != "f64":
        import oracle as O

        m64 = (1 << 64) - 1
        return np.array([O.gamma_unit(shape, seed, (gid0 + i) & m64, step, "f32") for i in range(n)])
    lo, hi = H._gid_words(gid0, n)
    k0, k1 = H._key(seed)
    dd = shape - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * dd)
    out = np.full(n, dd)
    open_ = np.ones(n, dtype=bool)
    for a in range(8):
        w = S.philox4x32_10(lo, hi, step, TAG_GAMMA | a, k0, k1)
        ur = (w[0].astype(np.float64) + 0.5) * H._TWO_M32
        ut = (w[1].astype(np.float64) + 0.5) * H._TWO_M32
        z = np.sqrt(-2.0 * np.log(ur)) * np.cos(2.0 * np.pi * ut)
        u = S.u01(w[2], w[3])
        v = 1.0 + c * z
        ok = v > 0.0
        v3 = np.where(ok, v, 1.0) ** 3
        hit = open_ & ok & (np.log(u) < 0.5 * z * z + dd - dd * v3 + dd * np.log(v3))
        out[hit] = dd * v3[hit]
        open_ &= ~hit
    return out


# ---- densities -----------------------------------------------------------------------------------------------------------------
def mix_logpdf(mix, x):
    """log sum_c exp(logw_c - 1/2 sum_j prec_cj (x_j - mu_cj)^2) in x's float type; C = 1 without exp / log; every term -inf or
    NaN: their sum (never -inf for a NaN row), as csrc mixture_eval and oracle.Mixture.logpdf."""
    ft = x.dtype.type
    logw, mu, prec = (np.asarray(a, dtype=x.dtype) for a in mix)
    mu, prec = np.atleast_2d(mu), np.atleast_2d(prec)
    C = len(logw)
    terms = np.empty((x.shape[0], C), dtype=x.dtype)
    with np.errstate(all="ignore"):
        for c in range(C):
            t = x - mu[c]
            terms[:, c] = logw[c] - ft(0.5) * (t * t * prec[c]).sum(-1)
        if C == 1:
            return terms[:, 0]
        m = np.nanmax(np.where(np.isnan(terms), -np.inf, terms), axis=1)
        dead = m == -np.inf
        ms = np.where(dead, ft(0.0), m)
        val = ms + np.log(np.exp(terms - ms[:, None]).sum(axis=1))
        return np.where(dead, terms.sum(axis=1), val)


def log_p_t(ll, lp, lq, beta, guard=True):
    """(1 - beta) lq + beta (ll + lp); +inf or NaN becomes -inf (the guard of asmc_pcn_dev.h log_p_t)."""
    ft = np.asarray(ll).dtype.type
    with np.errstate(all="ignore"):
        r = ft(1.0 - beta) * lq + ft(beta) * (ll + lp)
    return np.where(r < np.inf, r, -np.inf) if guard else r


def ref_corr(q, nu, d):
    """Minus the log-density of the reference at |y|^2 = q up to a constant: q/2, or ((d + nu)/2) log(1 + q/nu) (nu > 0)."""
    ft = q.dtype.type
    if nu > 0.0:
        return ft(0.5) * (ft(d) + ft(nu)) * np.log1p(q / ft(nu))
    return ft(0.5) * q


def _store(a, store, ft):
    """Round to the storage type and widen again (what the kernels do wherever a value goes to the state)."""
    return a if store is None else a.astype(store).astype(ft)


def _tri(M, ft):
    return np.tril(np.asarray(M, dtype=np.float64)).astype(ft)


# ---- one step ------------------------------------------------------------------------------------------------------------------
def propose(x, mu, L, Linv, rho, seed, gid0, step, nu=0.0, mode="f64", ft=np.float64, store=np.float64, y=None, bug=None,
            draws=None, round_y1=False):
    """The proposal half.  `x` [n, d] (or, with `y`, the whitened state itself: no whitening, and y' is rounded to the storage
    type as the whitened-state kernels round it).  `draws`: (xi, u) or (xi, u, Gamma variates) to use instead of the step's own.
    Returns a dict: y, y1, x1 (x', rounded to `store`), q0, q1, rs, log_u."""
    n, d = (x if y is None else y).shape
    ft = np.dtype(ft).type
    mu_, L_, Li_ = np.asarray(mu, dtype=ft), _tri(L, ft), _tri(Linv, ft)
    if y is None:
        y0 = (np.asarray(x).astype(ft) - mu_) @ Li_.T
    else:
        y0 = np.asarray(y).astype(ft)
    q0 = (y0 * y0).sum(axis=1)
    xi, u, g = (tuple(draws) + (None,))[:3] if draws is not None else noise(seed, gid0, n, step, d, mode) + (None,)
    if bug == "u_tile_local":  # keyed by the row's index inside its 64-row tile instead of gid0 + i
        u = np.concatenate([H.accept_uniforms(seed, gid0, min(64, n - r), step) for r in range(0, n, 64)])
    if nu > 0.0:
        shape = 0.5 * ((pad_dim(d) if bug == "shape_padded" else d) + nu)
        if g is None:
            g = gamma_unit(shape, seed, gid0, n, step, mode)
        rs = ft(rho) * np.sqrt((ft(nu) + q0) / (ft(2.0) * g.astype(ft)))
    else:
        rs = np.full(n, ft(rho))
    a = ft(1.0) - ft(rho) * ft(rho)
    if bug != "a_no_root":
        a = np.sqrt(a)
    y1 = a * y0 + rs[:, None] * xi.astype(ft)
    if y is not None or round_y1:  # (round_y1: the matrix-core kernels round y' in their proposal mode as well)
        y1 = _store(y1, store, ft)
    q1 = (y1 * y1).sum(axis=1)
    if bug == "q1_padded" and pad_dim(d) > d:  # the padded coordinates' noise counted into |y'|^2
        xp = noise(seed, gid0, n, step, pad_dim(d), mode)[0][:, d:].astype(ft)
        q1 = q1 + ((rs[:, None] * xp) ** 2).sum(axis=1)
    x1 = _store(mu_ + y1 @ L_.T, store, ft)
    return dict(y=y0, y1=y1, x1=x1, q0=q0, q1=q1, rs=rs, log_u=np.log(u.astype(ft)))


def accept(p, ll, lp, lq, nll, nlp, nlq, beta, nu, d, logj=None, logj_new=None, bug=None):
    """The decision half on a dict from `propose`: adds log_a, margin = log_a - log u and accept = log u < log_a."""
    guard = bug != "no_guard"
    with np.errstate(all="ignore"):
        lpn, lpo = log_p_t(nll, nlp, nlq, beta, guard), log_p_t(ll, lp, lq, beta, guard)
        if logj is not None:  # the second guard: the Jacobian term can turn a finite value into +inf or NaN
            lpn, lpo = lpn + logj_new, lpo + logj
            lpn, lpo = np.where(lpn < np.inf, lpn, -np.inf), np.where(lpo < np.inf, lpo, -np.inf)
        c1, c0 = ref_corr(p["q1"], nu, d), ref_corr(p["q0"], nu, d)
        log_a = (lpn - c1) - (lpo - c0) if bug == "corr_sign" else (lpn + c1) - (lpo + c0)
        p["log_a"], p["margin"] = log_a, log_a - p["log_u"]
        p["accept"] = p["log_u"] < log_a
    return p


def step(x, ll, lp, lq, beta, mu, L, Linv, rho, mixes, seed, gid0, step, nu=0.0, mode="f64", ft=np.float64, store=np.float64,
         bug=None, draws=None):
    """One fused x-state step (asmc_pcn_mutate, n_steps = 1 .. 3 at d <= 32): returns (x, ll, lp, lq) after the step - new arrays
    in the float type `ft` - and the per-row record of `propose` / `accept`."""
    ft = np.dtype(ft).type
    xf = np.asarray(x).astype(ft)
    c = [np.asarray(v).astype(ft) for v in (ll, lp, lq)]
    p = propose(xf, mu, L, Linv, rho, seed, gid0, step, nu, mode, ft, store, bug=bug, draws=draws)
    new = [mix_logpdf(m, p["x1"]) for m in mixes]
    accept(p, *c, *new, beta, nu, xf.shape[1], bug=bug)
    acc = p["accept"].copy()
    if bug == "ragged_last_lane" and len(acc) % 64:
        acc[-1] = False
    out = [np.where(acc[:, None], p["x1"], xf)] + [np.where(acc, nv, ov) for nv, ov in zip(new, c)]
    p["new"] = new
    return out, p


# ---- the step loops of asmc_pcn_mutate ----------------------------------------------------------------------------------------
def adapt_rho(rho, count, n, target, t):
    """asmc_pcn_dev.h pcn_adapt_rho: log rho += (acc - target) / (t + 1)^0.75, clipped to [1e-4, 0.99]."""
    r = float(np.exp(np.log(rho) + (count / n - target) / (t + 1) ** 0.75))
    return min(max(r, 1e-4), 0.99)


def adapt_schedule(rho, counts, n, target, adapt):
    """(rho_hist, rho_out) for the accept counts of a call's steps; adapt = 0 off, 1 after every step, k >= 2 lagged: the step
    size is held for blocks of k steps and the block's updates are replayed in order at its end or at the call's last step
    (k_pcn_adapt).  The counts must be those the held step sizes produce: see `mutate`."""
    hist, r = [], rho
    for t, c in enumerate(counts):
        hist.append(r)
        r = next_rho(r, counts, t, n, target, adapt, t == len(counts) - 1)
    return np.array(hist), r


def rho_tol(rho_hist):
    """Relative tolerance of an adapted step size against `adapt_schedule`: an update is exp(log rho + delta)
    with delta from one division, one power and one subtraction; each within an ulp in either libm, the exponent carries an
    absolute error of (|log rho| + 2) 2^-52, which exp turns into as much relative error, plus its own ulp - summed over the
    call's updates."""
    return float(sum(abs(np.log(r)) + 3.0 for r in rho_hist) * EPS64)


def next_rho(rho, counts, t, n, target, adapt, last):
    if adapt == 0:
        return rho
    if adapt == 1:
        return adapt_rho(rho, counts[t], n, target, t)
    if (t + 1) % adapt == 0 or last:
        for tp in range(t - t % adapt, t + 1):
            rho = adapt_rho(rho, counts[tp], n, target, tp)
    return rho


def mutate(x, ll, lp, lq, beta, mu, L, Linv, rho, mixes, seed, gid0, n_steps, step0=0, nu=0.0, mode="f64", ft=np.float64,
           store=np.float64, state="x", target=0.234, adapt=0, draws=None, split=False, logj=None, jac=None, jac_from=0):
    """n_steps steps as asmc_pcn_mutate runs them.  state = "x": every step whitens, proposes and un-whitens (the register
    kernels' x-state loop and the generic kernel); state = "y": the whitened state is kept, ROUNDED TO THE STORAGE TYPE, between
    the steps, and x and the three carried densities are re-evaluated from it at the end (coordinate-major, row-major and
    matrix-core whitened paths).  `draws(step)`: the step's draws as `propose` takes them, instead of its own.
    split = True (with state = "y"): the asmc_pcn_ysplit_* session - the caller evaluates the densities at the stored x' between
    propose and accept and they are carried as they are, nothing is re-evaluated at the end; from step index `jac_from` on the
    carried log-Jacobian `logj` and jac(x') join the log-target (the second guard) and follow the accepted state.
    Returns a dict: x, ll, lp, lq (lj), counts, rho_hist, rho, and `margins` [n_steps, n]."""
    ft = np.dtype(ft).type
    xf = np.asarray(x).astype(ft)
    c = [np.asarray(v).astype(ft) for v in (ll, lp, lq)]
    n, d = xf.shape
    mu_, L_, Li_ = np.asarray(mu, dtype=ft), _tri(L, ft), _tri(Linv, ft)
    y = _store((xf - mu_) @ Li_.T, store, ft) if state == "y" else None
    lj = None if logj is None else np.asarray(logj).astype(ft)
    counts, hist, margins, r = [], [], [], float(rho)
    for t in range(n_steps):
        hist.append(r)
        dr = None if draws is None else draws(step0 + t)
        if state == "y":
            p = propose(None, mu, L, Linv, r, seed, gid0, step0 + t, nu, mode, ft, store, y=y, draws=dr)
        else:
            p = propose(xf, mu, L, Linv, r, seed, gid0, step0 + t, nu, mode, ft, store, draws=dr)
        new = [mix_logpdf(m, p["x1"]) for m in mixes]
        if lj is not None and t >= jac_from:
            ljn = jac(p["x1"])
            accept(p, *c, *new, beta, nu, d, lj, ljn)
            lj = np.where(p["accept"], ljn, lj)
        else:
            accept(p, *c, *new, beta, nu, d)
        acc = p["accept"]
        if state == "y":
            y = np.where(acc[:, None], p["y1"], y)
        else:
            xf = np.where(acc[:, None], p["x1"], xf)
        c = [np.where(acc, nv, ov) for nv, ov in zip(new, c)]
        counts.append(int(acc.sum()))
        margins.append(p["margin"])
        r = next_rho(r, counts, t, n, target, int(adapt), t == n_steps - 1)
    if state == "y":
        xf = _store(mu_ + y @ L_.T, store, ft)
        if not split:
            c = [mix_logpdf(m, xf) for m in mixes]
    return dict(x=xf, ll=c[0], lp=c[1], lq=c[2], lj=lj, counts=np.array(counts), rho_hist=np.array(hist), rho=r,
                margins=np.array(margins))


# ---- tolerances and the comparison the device tests use ----------------------------------------------------------------------
# DESIGN.md §3.19.  The unit of a quantity is the float64 restatement's worst row error against its own longdouble run on the case's
# inputs, floored at the first-order rounding bound of a length-d dot product (a lucky case must not shrink the tolerance to
# nothing); the device gets MULT units.
MULT = 16.0


def units(ref64, refld, d, store=np.float64):
    """{"x", "c", "m"}: units of positions (relative to 1 + |x|), carried densities (relative to 1 + |value|) and accept margins
    (absolute) from a float64 and a longdouble result of `mutate` / `step` (dicts with x, ll, lp, lq, margins).  fp32 storage:
    the two runs may round a coordinate to neighbouring floats, so a position is good to one float32 spacing and the densities to
    what that spacing moves them (the caller passes the first-order bound through `units_fp32`)."""
    with np.errstate(all="ignore"):
        ux = np.nanmax(np.abs(ref64["x"] - refld["x"]) / (1 + np.abs(refld["x"])))
        uc = max(_relerr(ref64[k], refld[k]) for k in ("ll", "lp", "lq"))
        dm = np.abs(ref64["margins"] - refld["margins"])
        um = float(np.nanmax(np.where(np.isfinite(dm), dm, 0.0)))
    floor = d * EPS64
    return dict(x=max(float(ux), floor), c=max(float(uc), floor), m=max(um, floor))


def _relerr(a, b):
    fin = np.isfinite(a) & np.isfinite(b)
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(a[fin] - b[fin]) / (1 + np.abs(b[fin]).astype(np.float64))))


def fp32_density_shift(mixes, x):
    """First-order bound on what rounding every coordinate of x to float32 moves any of the three densities by, worst row:
    sum_j max_c |prec_cj (x_j - mu_cj)| * 2^-24 |x_j| (a mixture's gradient is a convex combination of its components')."""
    worst = 0.0
    x = np.asarray(x, dtype=np.float64)
    for logw, mu, prec in mixes:
        g = np.max(np.abs(np.atleast_2d(prec)[None] * (x[:, None, :] - np.atleast_2d(mu)[None])), axis=1)
        worst = max(worst, float(np.max((g * (0.5 * EPS32) * np.abs(x)).sum(axis=1))))
    return worst


def razor(margins, tol_m):
    """Rows whose decision the reference cannot call at some step: |log_a - log u| <= tol_m.  `margins` [n_steps, n] or [n]; a NaN
    margin (both log-targets -inf) is a decided rejection."""
    m = np.atleast_2d(np.asarray(margins, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        return np.any(np.abs(m) <= tol_m, axis=0)


def razor_cap(n):
    """At most 0.5 % of a case's rows may be undecided, and at most 2 for cases of n <= 257 rows."""
    return 2 if n <= 257 else int(0.005 * n)


WORST = {}  # label -> [worst position error / tol_x, worst density error / tol_c] over the comparisons made (what DESIGN.md quotes)


def compare(got, ref, margins, tol_x, tol_c, tol_m, label=None):
    """The comparison of tests/test_gpu_pcn.py: `got` and `ref` are dicts with x, ll, lp, lq after the same step(s).  Rows inside
    the razor band are skipped (and must stay within razor_cap); every other row must agree in position - which is agreement in
    every decision, a proposal being rho * O(1) away - and in the three carried densities, non-finite values exactly.  Returns
    the number of undecided rows; raises AssertionError otherwise."""
    n = len(ref["x"])
    und = razor(margins, tol_m)
    assert und.sum() <= razor_cap(n), f"{und.sum()} of {n} rows inside the razor band of {tol_m:.3g}"
    ok = ~und
    gx, rx = np.asarray(got["x"], dtype=np.float64)[ok], np.asarray(ref["x"], dtype=np.float64)[ok]
    err = np.abs(gx - rx) / (1 + np.abs(rx))
    bad = np.flatnonzero(~(err <= tol_x).all(axis=1))
    w = WORST.setdefault(label, [0.0, 0.0])
    w[0] = max(w[0], float(np.nanmax(err, initial=0.0)) / tol_x)
    assert bad.size == 0, f"{bad.size} rows off in position (worst {np.nanmax(err):.3g}, tolerance {tol_x:.3g}); first: row {np.flatnonzero(ok)[bad[0]]}"
    for k in ("ll", "lp", "lq"):
        g, r = np.asarray(got[k], dtype=np.float64)[ok], np.asarray(ref[k], dtype=np.float64)[ok]
        fin = np.isfinite(r)
        assert np.array_equal(np.isfinite(g), fin), f"{k}: finite / non-finite pattern differs"
        assert np.array_equal(g[~fin], r[~fin], equal_nan=True), f"{k}: non-finite values differ"
        e = np.abs(g[fin] - r[fin]) / (1 + np.abs(r[fin]))
        w[1] = max(w[1], float(e.max(initial=0.0)) / tol_c)
        assert e.size == 0 or e.max() <= tol_c, f"{k}: worst error {e.max():.3g}, tolerance {tol_c:.3g}"
    return int(und.sum())


# ---- the shared case table ----------------------------------------------------------------------------------------------------
def problem(n, d, seed, C=1, store=np.float64):
    """A correlated reference (mu, L, Linv), three diagonal mixtures of C components (likelihood, prior, proposal) and n start
    points rounded to the storage type, with their densities: (x, ll, lp, lq, mu, L, Linv, mixes)."""
    g = np.random.default_rng(seed)
    A = g.normal(size=(d, d)) / np.sqrt(d)
    L = np.linalg.cholesky(A @ A.T + 0.5 * np.eye(d))
    Linv = np.linalg.inv(L)
    mu = 0.1 * g.normal(size=d)
    mixes = []
    for k in range(3):
        m = g.normal(size=(C, d)) * (0.5 if k < 2 else 0.0)
        v = g.uniform(0.7, 1.5, size=(C, d)) * (2.25 if k == 2 else 1.0)
        lw = np.log(np.full(C, 1.0 / C)) - 0.5 * d * np.log(2 * np.pi) - 0.5 * np.log(v).sum(1)
        mixes.append((lw, m, 1 / v))
    x = (1.5 * g.normal(size=(n, d))).astype(store).astype(np.float64)  # (drawn last: a smaller n is a prefix of the same problem)
    ll, lp, lq = (mix_logpdf(mx, x) for mx in mixes)
    return x, ll, lp, lq, mu, np.tril(L), np.tril(Linv), mixes


def case_state(d, n_steps, C, env=None):
    """Which form of the state asmc_pcn_mutate steps on (the dispatch of pcn_mutate_impl, csrc/asmc_pcn_drive.hip): the matrix-core widths always whiten;
    the register widths whiten for n_steps >= 4 - mixtures only on the coordinate-major kernels - unless ASMC_PCN_XSTATE is set;
    the generic kernel never does.  A zero-padded problem follows its padded width."""
    if env in ("ASMC_PCN_GENERIC", "big", "offset") or (env == "ASMC_PCN_NOPAD" and pad_dim(d) != d):
        return "x"  # (every case of the table with one of these runs on the generic kernel)
    if env == "session":
        return "y"
    D = pad_dim(d)
    if D in (64, 128):
        return "y"
    if D > 128:
        return "x"
    if n_steps >= 4 and env != "ASMC_PCN_XSTATE" and not (env == "ASMC_PCN_AOS" and C > 1):
        return "y"
    return "x"


def _case(d, n, C=1, nu=0.0, n_steps=1, store="f64", mode="f64", env=None, seed=1, offset=0, rho=0.4, beta=0.37):
    return dict(d=d, n=n, C=C, nu=nu, n_steps=n_steps, store=store, mode=mode, env=env, seed=seed, offset=offset, rho=rho,
                beta=beta)


def case_id(c):
    return "d{d}-n{n}-C{C}-nu{nu:g}-s{n_steps}-{store}-{mode}-{env}-o{offset}".format(**c)


def _cases():
    out = []
    # the dispatch axes of the register kernels: x-state, coordinate-major whitened single and mixture
    for d in (4, 8, 16, 32):
        for nu in (0.0, 5.5):
            for n_steps in (1, 4):
                for C in (1, 3):
                    for store, mode in (("f64", "f64"), ("f32", "f64"), ("f64", "f32"), ("f32", "f32")):
                        out.append(_case(d, 257, C, nu, n_steps, store, mode))
                    if n_steps == 4:
                        out.append(_case(d, 257, C, nu, n_steps, env="ASMC_PCN_XSTATE"))  # the x-state loop of four steps
                        for store, mode in (("f64", "f64"), ("f32", "f64"), ("f64", "f32"), ("f32", "f32")):  # row-major whitened state
                            if C == 1 or (store, mode) == ("f64", "f64"):  # (a mixture falls back to the x-state loop)
                                out.append(_case(d, 257, C, nu, n_steps, store, mode, env="ASMC_PCN_AOS"))
    # ragged tiles of the register kernels (one block holds four wave tiles), and one population for the acceptance rate
    for n in (1, 63, 64, 65, 255, 256, 3001):
        out.append(_case(8, n, nu=5.5 if n % 2 else 0.0))
    # zero-padded problems: Gamma shape and both |y|^2 on the real d
    for d in (1, 3, 5, 9, 15, 17, 31, 33, 63, 65, 127):
        out.append(_case(d, 130, C=2 if d % 4 == 1 else 1, nu=5.5 if d % 3 else 0.0, n_steps=1 if d % 2 else 4))
    # matrix-core kernels: groups of 16 rows, 8 waves per block
    for d in (64, 128):
        for n, C, nu, steps, store, mode in ((1, 1, 5.5, 1, "f64", "f64"), (15, 1, 5.5, 1, "f64", "f32"), (16, 1, 0.0, 1, "f32", "f64"),
                                             (17, 3, 5.5, 1, "f32", "f32"), (127, 1, 0.0, 1, "f32", "f32"), (128, 1, 0.0, 1, "f64", "f32"),
                                             (129, 1, 5.5, 1, "f32", "f64"), (1999, 3, 0.0, 2, "f64", "f64"), (130, 2, 5.5, 2, "f64", "f64")):
            out.append(_case(d, n, C, nu, steps, store, mode))
    # the generic LDS kernel.  A width with kernels of its own reaches it when x is not 16-byte aligned (an offset view):
    # 64-byte rows 8 bytes off (VEC = 8), fp32 rows 4 and 8 bytes off (VEC = 4, 8)
    for n in (1, 63, 64, 65, 255, 256, 257):
        out.append(_case(8, n, nu=5.5 if n % 2 else 0.0, offset=1, mode="f32" if n in (64, 255) else "f64", seed=3))
    out.append(_case(4, 130, 3, 5.5, 2, "f32", "f64", offset=1))
    out.append(_case(16, 130, 1, 0.0, 2, "f32", "f32", offset=2))
    out.append(_case(64, 65, 2, 5.5, 1, "f64", "f64", offset=1))
    # ... every width above 128 (an engine with d_max = 256 pads nothing: 33 goes there too) ...
    for n, store, mode, nu, C in ((65, "f64", "f64", 0.0, 1), (257, "f64", "f32", 5.5, 2), (130, "f32", "f64", 5.5, 1),
                                  (63, "f32", "f32", 0.0, 3)):
        out.append(_case(140, n, C, nu, 2, store, mode, env="big"))
    out.append(_case(33, 130, 2, 5.5, 4, env="big"))
    # ... and everything under the two environment switches
    for d in (5, 33):
        for env in ("ASMC_PCN_NOPAD", "ASMC_PCN_GENERIC"):
            out.append(_case(d, 130, 2, 5.5, 2, env=env, mode="f32" if d == 33 else "f64"))
    out.append(_case(32, 130, 1, 5.5, 4, env="ASMC_PCN_GENERIC", mode="f32"))
    out.append(_case(128, 65, 1, 0.0, 1, "f32", env="ASMC_PCN_GENERIC"))
    # (appended, so that the cases above keep their seeds) the x-state loop of four steps in the other storage and noise types
    for d in (4, 8, 16, 32):
        for nu in (0.0, 5.5):
            for C in (1, 3):
                for store, mode in (("f32", "f64"), ("f64", "f32"), ("f32", "f32")):
                    out.append(_case(d, 257, C, nu, 4, store, mode, env="ASMC_PCN_XSTATE"))
    # the whitened-state split session (asmc_pcn_ysplit_*) at every width it accepts: two steps, the second with log-Jacobians
    for d in SESSION_DIMS:
        for store, mode in (("f64", "f64"), ("f32", "f64"), ("f64", "f32"), ("f32", "f32")):
            out.append(dict(_case(d, 257, 2, 5.5 if (d in (8, 32)) != (mode == "f32") else 0.0, 2, store, mode, env="session"), split=True))
    for k, c in enumerate(out):
        c["state"] = case_state(c["d"], c["n_steps"], c["C"], "offset" if c["offset"] else c["env"])
        # one seed per case: the library keeps the last Gamma draw by (n, seed, gid0, shape, noise, step), and a case that found
        # another's variates there would launch one kernel fewer than its path says
        c["seed"] = c["seed"] + 7 * c["d"] + c["n"] + 1000 * k + RESEED.get(case_id(c), 0)
    return out


# cases whose first seed left more rows inside the razor band than razor_cap allows (tests/test_pcn_ref.py): another seed, the same cap
RESEED = {}


CASES = _cases()
STORE = {"f64": np.float64, "f32": np.float32}


def jittered_draws(seed, gid0, n, d, nu, mode, jitter):
    """draws(step) for `mutate`: the step's own normals each moved by +-jitter (signs from a generator of their own) and its Gamma
    variate by what moving its normal by as much does to it, d log g / dz = 3 c / (1 + c z) <= 1 / sqrt(shape - 1/3) - the
    perturbation that measures the unit of the f32 noise mode (case_tolerances); the restatement itself knows nothing of it."""
    def draws(step):
        xi, u = noise(seed, gid0, n, step, d, mode)
        sg = np.random.default_rng(step).choice([-1.0, 1.0], size=(n, d + 1)) * jitter
        g = None
        if nu > 0.0:
            shape = 0.5 * (d + nu)
            g = gamma_unit(shape, seed, gid0, n, step, mode) * (1.0 + sg[:, d] / np.sqrt(shape - 1.0 / 3.0))
        return xi + sg[:, :d], u, g

    return draws


def sin_jac(x):
    """A smooth function of the proposal that stands in for a log-Jacobian, with +inf planted where the second guard must act."""
    with np.errstate(all="ignore"):
        v = x.dtype.type(0.3) * np.sin(x).sum(axis=1)
    return np.where(np.arange(len(v)) % 17 == 5, np.inf, v)


def run_case(c, ft=np.float64, jitter=None):
    """The case's inputs and the restatement's result in the float type `ft` (jitter: with `jittered_draws`)."""
    st = STORE[c["store"]]
    x, ll, lp, lq, mu, L, Linv, mixes = problem(c["n"], c["d"], c["seed"], c["C"], st)
    seed = 4242 + c["seed"]
    draws = None if jitter is None else jittered_draws(seed, 1000, c["n"], c["d"], c["nu"], c["mode"], jitter)
    kw = {}
    if c.get("split"):  # the session: step 0 without log-Jacobians, from step 1 on with them
        kw = dict(split=True, logj=session_logj(c), jac=sin_jac, jac_from=1)
    ref = mutate(x, ll, lp, lq, c["beta"], mu, L, Linv, c["rho"], mixes, seed, 1000, c["n_steps"], 5, c["nu"],
                 c["mode"], ft, st, c["state"], draws=draws, **kw)
    return (x, ll, lp, lq, mu, L, Linv, mixes), ref


def session_logj(c):
    return np.random.default_rng(c["seed"] + 1).normal(size=c["n"])


XI32 = 6.7 * EPS32  # one float32 spacing at the largest normal the fp32 Box-Muller can return


def case_tolerances(c, inputs, ref64, refld, ref_jit=None):
    """(tol_x, tol_c, tol_m) of a case: MULT units.
    fp32 storage: the device and the restatement may round a value that goes to the state to neighbouring floats, so a position
    is good to one float32 spacing more - through L, once per step, where the whitened state is what is stored - and a density
    or a margin to what that spacing moves them (first order, fp32_density_shift).
    f32 noise: the hardware's transcendentals against the libm restatement of the same fp32 formula.  Its unit is what moving
    every normal by one float32 spacing at the largest normal (XI32; the Gamma variate by its derivative times that) does to the
    float64 restatement: `ref_jit` = run_case(c, jitter=XI32), compared on the rows whose decisions it leaves alone."""
    u = units(ref64, refld, c["d"])
    tx, tc, tm = MULT * u["x"], MULT * u["c"], MULT * u["m"]
    if c["mode"] == "f32":
        same = np.all((ref64["margins"] > 0) == (ref_jit["margins"] > 0), axis=0)
        j = units({k: (v[:, same] if k == "margins" else v[same]) for k, v in ref64.items() if k in ("x", "ll", "lp", "lq", "margins")},
                  {k: (v[:, same] if k == "margins" else v[same]) for k, v in ref_jit.items() if k in ("x", "ll", "lp", "lq", "margins")}, 0)
        tx, tc, tm = tx + MULT * j["x"], tc + MULT * j["c"], tm + MULT * j["m"]
    if c["store"] == "f32":
        steps = c["n_steps"] if c["state"] == "y" else 1
        through = float(np.abs(inputs[5]).sum(axis=1).max()) if c["state"] == "y" else 1.0
        shift = fp32_density_shift(inputs[7], ref64["x"]) * steps * through
        tx, tc, tm = tx + EPS32 * steps * through, tc + 2 * shift, tm + 8 * shift
    return tx, tc, tm


def case_reference(c):
    """(inputs, float64 result, (tol_x, tol_c, tol_m)) of a case; cached: the device tests and the condition check share it."""
    key = case_id(c)
    if key not in _REF:
        inputs, r64 = run_case(c)
        n_ld = min(c["n"], 2048)  # (the longdouble run of the one large case: its first rows)
        if n_ld < c["n"]:
            sub = dict(c, n=n_ld)
            rld = run_case(sub, np.longdouble)[1]
            r64s = run_case(sub)[1]
        else:
            rld, r64s = run_case(c, np.longdouble)[1], r64
        jit = run_case(dict(c, n=n_ld), jitter=XI32)[1] if c["mode"] == "f32" else None
        _REF[key] = (inputs, r64, case_tolerances(c, inputs, r64s, rld, jit))
    return _REF[key]


_REF = {}
