"""Host restatement of the preconditioning transforms (include/asmc.h asmc_transform_forward / _inverse, csrc/asmc_transform.hip).

`composite` follows the reference's CompositeTransform operation by operation (transforms.py:270-316 over the periodic wrap :411-436,
the unit-interval maps :476-512, probit :548-566, logit :591-601 with utils.py:196-245, affine :629-638), written once for two float
types:

* `np.float64`: numpy / scipy elementary functions, `np.clip`, `np.mod` - the reference's own arithmetic, bit for bit.
* `np.longdouble`: plain arithmetic in long double, every elementary function from mpmath at 50 digits.  Only the inputs, the table
  entries and the clamp ends eps and fl(1 - eps) - for the probit, of erfinv's argument: fl(2 eps - 1), fl(2 fl(1 - eps) - 1) - are
  fp64 by definition; sqrt(2) and log(2 pi) are the true constants.  The inverse
  logit's Jacobian term is the analytic -|v| - 2 log(1 + e^-|v|) away from the clamp (the reference's log u + log1p(-u) on the
  rounded u cancels next to u = 1) and log u + log1p(-u) on the fp64 clamp end where the clamp engages.

The gap between the two runs is the conditioning of the expression plus the error of numpy's own functions; the device tests allow
a multiple of it (tests/test_gpu_transforms.py).  The edge-value sets of those tests live here too, so that the CPU tests
(tests/test_transform_ref.py) can pin the restatement against the C oracle on the very same inputs.  A test helper: the product
never imports it.
"""
from __future__ import annotations

import math

import mpmath
import numpy as np
from scipy import special as _sp

LD = np.longdouble
_MP = mpmath.mp.clone()
_MP.dps = 50


# ---- the two sets of elementary functions ----------------------------------------------------------------------------------------
class _F64:
    log, log1p, exp, erf, erfinv = np.log, np.log1p, np.exp, _sp.erf, _sp.erfinv
    sqrt2 = math.sqrt(2)  # (the reference's own constants: transforms.py:553-562)
    log_2pi = math.log(2 * math.pi)


def _to_mp(v):
    hi = float(v)
    return _MP.mpf(hi) + _MP.mpf(float(v - LD(hi)))


def _from_mp(m):
    hi = float(m)
    if not math.isfinite(hi) or hi == 0.0:
        return LD(hi)
    return LD(hi) + LD(float(m - _MP.mpf(hi)))


def _lift(mp_fn, np_fn):
    """Elementwise long-double function: mpmath where the argument is finite and in the function's domain, IEEE special values
    (numpy's, on the fp64-rounded argument) everywhere else - log(0) = -inf, erfinv(1) = inf, f(NaN) = NaN."""

    def one(v):
        if np.isfinite(v):
            try:
                r = mp_fn(_to_mp(v))
                if isinstance(r, _MP.mpf) and _MP.isfinite(r):
                    return _from_mp(r)
            except (ValueError, ZeroDivisionError, OverflowError):
                pass
        with np.errstate(all="ignore"):
            return LD(np_fn(np.float64(v)))

    def f(a):
        a = np.asarray(a, dtype=LD)
        out = np.empty(a.shape, dtype=LD)
        flat = out.reshape(-1)
        for i, v in enumerate(a.reshape(-1)):
            flat[i] = one(v)
        return out

    return f


class _HP:
    log = staticmethod(_lift(_MP.log, np.log))
    log1p = staticmethod(_lift(_MP.log1p, np.log1p))
    exp = staticmethod(_lift(_MP.exp, np.exp))
    erf = staticmethod(_lift(_MP.erf, _sp.erf))
    erfinv = staticmethod(_lift(_MP.erfinv, _sp.erfinv))
    sqrt2 = _from_mp(_MP.sqrt(2))
    log_2pi = _from_mp(_MP.log(2 * _MP.pi))


def _funcs(ft):
    if ft is np.float64:
        return _F64
    assert ft is LD and np.finfo(LD).nmant >= 63, "the high-precision run needs an extended long double"
    return _HP


def constants(kind, lower, upper, std=None, ft=np.float64):
    """(unit_logj, affine_logj) of include/asmc.h's asmc_transform, forward sign: -sum log(upper - lower) over the bounded block
    (transforms.py:474) and -sum log|std| (:621)."""
    F = _funcs(ft)
    bnd = np.asarray(kind) != 0
    lo, up = np.asarray(lower, dtype=np.float64).astype(ft), np.asarray(upper, dtype=np.float64).astype(ft)
    unit = -F.log(up[bnd] - lo[bnd]).sum() if bnd.any() else ft(0.0)
    aff = ft(0.0) if std is None else -F.log(np.abs(np.asarray(std, dtype=np.float64).astype(ft))).sum()
    return unit, aff


def composite(x, kind, periodic, lower, upper, mean=None, std=None, eps=1e-6, inverse=False, ft=np.float64):
    """(y [n, d], log|det J| [n], terms [n, d]) of CompositeTransform.forward (inverse=False) or .inverse on the rows of x, in
    float type `ft`.  kind[j]: 0 none, 1 logit, 2 probit (one bounded kind per table, as in the reference); periodic[j]: wrap into
    [lower, upper); mean / std None: no affine stage.  terms holds the bounded block's element terms of log|det J| (0 elsewhere);
    the row value adds the constants of `constants` in the reference's grouping."""
    F = _funcs(ft)
    x = np.atleast_2d(np.asarray(x, dtype=np.float64)).astype(ft)
    kind, periodic = np.asarray(kind), np.asarray(periodic)
    per, bnd = periodic != 0, kind != 0
    probit = bool((kind == 2).any())
    assert not (probit and (kind == 1).any()), "one bounded transform per composite"
    lo, up = np.asarray(lower, dtype=np.float64).astype(ft), np.asarray(upper, dtype=np.float64).astype(ft)
    affine = mean is not None
    if affine:
        mean, std = np.asarray(mean, dtype=np.float64).astype(ft), np.asarray(std, dtype=np.float64).astype(ft)
    unit, aff = constants(kind, lower, upper, std if affine else None, ft)
    c_lo, c_hi = ft(np.float64(eps)), ft(np.float64(1.0) - np.float64(eps))  # the clamp ends: fp64 by definition
    half = ft(0.5)
    terms = np.zeros(x.shape, dtype=ft)
    lj = np.zeros(x.shape[0], dtype=ft)

    def wrap(x):
        x[:, per] = lo[per] + np.mod(x[:, per] - lo[per], up[per] - lo[per])

    with np.errstate(all="ignore"):
        if not inverse:
            if per.any():
                wrap(x)
            if bnd.any():
                u = (x[:, bnd] - lo[bnd]) / (up[bnd] - lo[bnd])
                u = np.clip(u, c_lo, c_hi)
                if probit:
                    # the clamp ends of erfinv's argument are fp64 by definition too: fl(2 c - 1).  erfinv amplifies that
                    # rounding 1e5-fold at eps = 1e-6, and a clamped coordinate maps to a constant, not to a computation
                    # (a no-op in fp64)
                    e_lo, e_hi = (ft(np.float64(2.0) * np.float64(c) - np.float64(1.0)) for c in (c_lo, c_hi))
                    y = F.erfinv(np.where(u == c_lo, e_lo, np.where(u == c_hi, e_hi, 2 * u - 1))) * F.sqrt2
                    t = half * (F.log_2pi + y**2)
                    rows = half * (F.log_2pi + y**2).sum(-1)
                else:
                    a, b = F.log(u), F.log1p(-u)
                    y = a - b
                    t = -a - b
                    rows = t.sum(-1)
                x[:, bnd], terms[:, bnd] = y, t
                lj += rows + unit
            if affine:
                x = (x - mean) / std
                lj += aff
        else:
            if affine:
                x = x * std + mean
                lj += -aff
            if bnd.any():
                v = x[:, bnd]
                if probit:
                    t = -(half * (F.log_2pi + v**2))
                    rows = t.sum(-1)
                    u = half * (1 + F.erf(v / F.sqrt2))
                else:
                    u0 = 1 / (1 + F.exp(-v))
                    u = np.clip(u0, c_lo, c_hi)
                    t = F.log(u) + F.log1p(-u)
                    if ft is not np.float64:
                        av = np.abs(v)
                        t = np.where((u0 < c_lo) | (u0 > c_hi), t, -av - 2 * F.log1p(F.exp(-av)))
                    rows = t.sum(-1)
                x[:, bnd], terms[:, bnd] = (up[bnd] - lo[bnd]) * u + lo[bnd], t
                lj += rows + (-unit)
            if per.any():
                wrap(x)
    return x, lj, terms


# ---- error measures ---------------------------------------------------------------------------------------------------------------
def ulp64(v):
    """Spacing of fp64 at |v| (v in any float type)."""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)))


def gap_ulps(a, hp, unit=None):
    """max |a - hp| in ulps of fp64 at hp (or in the given units) over the entries where hp is finite; 0 for an empty set."""
    hp = np.asarray(hp, dtype=LD)
    fin = np.isfinite(hp)
    if not fin.any():
        return 0.0
    unit = ulp64(hp) if unit is None else np.asarray(unit, dtype=np.float64)
    with np.errstate(all="ignore"):
        g = np.abs(np.asarray(a, dtype=np.float64).astype(LD) - hp)[fin] / np.broadcast_to(unit, hp.shape)[fin].astype(LD)
    return float(np.max(g))


def same_nonfinite(a, b):
    """NaN where b has NaN and the same +-inf."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.where(np.isinf(a), a, 0.0), np.where(np.isinf(b), b, 0.0)))


# ---- tables and inputs ------------------------------------------------------------------------------------------------------------
BOUNDS = ((0.0, 1.0), (-3.0, 2.5), (1e6, 1e6 + 1.0), (0.0, 1e-3))
PERIODS = ((0.0, 2.0 * math.pi), (-math.pi, math.pi))
# inverse logit arguments: below the clamp of eps = 1e-6 (it engages at |v| = 13.815509557963773), where next to it the reference's
# log1p(-u) cancels, and above it, where both ends are constants - separate groups, or the first's conditioning would hide the second
LOGIT_V = (0.0, 1e-300, 1e-8, 1.0, 13.7, 13.8155)
LOGIT_V_CLAMPED = (13.9, 36.0, 37.0, 40.0, 700.0, 709.8, 745.2, 800.0)
PROBIT_V = (0.0, 1e-8, 1.0, 4.7, 4.76, 5.5, 8.2, 8.3, 9.0, 38.0, 40.0)
EPS = 1e-6


def _cycle(pairs, d):
    lo = np.array([pairs[j % len(pairs)][0] for j in range(d)])
    up = np.array([pairs[j % len(pairs)][1] for j in range(d)])
    return lo, up


def affine_table(d, seed=0):
    """mean / std of mixed signs, magnitudes log-uniform in [1e-3, 1e3]."""
    g = np.random.default_rng(1000 + seed)
    mag = lambda: 10.0 ** g.uniform(-3, 3, size=d) * g.choice([-1.0, 1.0], size=d)  # noqa: E731
    return mag(), mag()


def bounded_edge_x(lo, up, eps=EPS):
    """[16, d]: every column runs through its own bounds' edge values."""
    w = up - lo
    rows = [lo, up, lo - w / 3, up + w / 3, np.nextafter(lo, up), np.nextafter(lo, -np.inf), np.nextafter(up, lo),
            np.nextafter(up, np.inf)]
    rows += [lo + w * f for f in (eps / 2, eps, 2 * eps, 1e-300)]
    rows += [up - w * f for f in (eps / 2, eps, 2 * eps)]
    rows += [lo + 0.5 * w]
    return np.array(rows)


def periodic_edge_x(lo, up):
    w = up - lo
    zero = np.zeros_like(lo)
    return np.array([lo, up, up + 1e-12 * w, lo - 1e-12 * w, lo + 1e6 * w + 0.3 * w, lo - 1e6 * w + 0.3 * w, zero, -zero])


def signed(vals, d):
    """[2 len(vals), d]: +v then -v, every column alike."""
    v = np.array(list(vals) + [-a for a in vals])
    return np.repeat(v[:, None], d, axis=1)


def table(name, d, seed=0, bounds=BOUNDS):
    """kind, periodic, lower, upper, mean, std of a named composition over d coordinates; the bounded coordinates cycle through
    `bounds`."""
    g = np.random.default_rng(seed + 17 * d)
    kind, per = np.zeros(d, dtype=np.int32), np.zeros(d, dtype=np.int32)
    lo, up = _cycle(bounds, d)
    mean = std = None
    if name in ("logit", "probit", "logit_affine", "probit_affine"):
        kind[:] = 1 if name.startswith("logit") else 2
    elif name == "periodic":
        per[:] = 1
        lo, up = _cycle(PERIODS, d)
    elif name in ("logit_mix", "probit_mix"):  # bounded / untouched / periodic coordinates side by side, with the affine stage
        r = g.integers(0, 3, size=d) if d > 2 else np.arange(d)
        kind[r == 0] = 1 if name == "logit_mix" else 2
        per[r == 2] = 1
        plo, pup = _cycle(PERIODS, d)
        lo, up = np.where(per == 1, plo, lo), np.where(per == 1, pup, up)
    else:
        assert name in ("none", "affine"), name
    if name.endswith(("affine", "mix")):
        mean, std = affine_table(d, seed)
    return kind, per, lo, up, mean, std


def interior_x(tab, n, inverse, seed=0, edges=False):
    """[n, d] inputs of a table: interior points (u in (0.001, 0.999), periodic coordinates up to half a period outside, |v| < 6 for
    the inverse; with the affine stage in front, the inverse's inputs are drawn in the stage's own units); edges=True overwrites
    scattered entries with finite edge values: on and outside the bounds, inside the clamp, far periods, and saturating inverse
    arguments."""
    kind, per, lo, up, mean, std = tab
    d = len(kind)
    g = np.random.default_rng(seed + n + 31 * d)
    w = up - lo
    if not inverse:
        x = np.where(per[None, :] == 1, lo + w * g.uniform(-0.5, 1.5, size=(n, d)), lo + w * g.uniform(0.001, 0.999, size=(n, d)))
        x = np.where(((kind == 0) & (per == 0))[None, :], 3.0 * g.normal(size=(n, d)), x)
        if edges:
            f = g.choice([0.0, 1.0, -0.3, 1.3, EPS / 2, 1 - EPS / 2, 2 * EPS, 1 - 2 * EPS, 1e6 + 0.3, -1e6 + 0.3], size=(n, d))
            x = np.where(g.uniform(size=(n, d)) < 0.15, lo + w * f, x)
        return x
    v = g.uniform(-6, 6, size=(n, d))
    if edges:
        e = g.choice([0.0, 1e-300, 14.5, 36.0, 37.0, 40.0, 700.0, 709.8, 745.2, 800.0], size=(n, d)) * g.choice([-1.0, 1.0], size=(n, d))
        v = np.where((g.uniform(size=(n, d)) < 0.15) & (kind != 0)[None, :], e, v)
    if mean is not None:  # so that v is what reaches the bounded stage, to rounding
        v = (v - mean) / std
    return v


NONFINITE = ((3, np.nan), (20, np.inf), (37, -np.inf))


def poke_nonfinite(x):
    """NaN, +inf and -inf in one coordinate each of rows 3, 20 and 37 (coordinates 0, 1 mod d, d - 1)."""
    x = np.array(x, dtype=np.float64)
    d = x.shape[1]
    for (row, val), col in zip(NONFINITE, (0, 1 % d, d - 1)):
        x[row, col] = val
    return x


def edge_cases(d):
    """{name: (table, x, inverse)}: one small case per (kind, direction, edge group) over d coordinates - for the bounded edge
    groups per interval as well - so that each group's tolerance is set by its own conditioning (with lower = 0 the inverse's tiny
    u is the value itself and its relative error is unbounded; next to lower = -3 it is not)."""
    cases = {}
    for k in ("logit", "probit"):
        for b, pair in enumerate(BOUNDS):
            tab = table(k, d, bounds=(pair,))
            cases[f"fwd_{k}_bounds{b}"] = (tab, bounded_edge_x(tab[2], tab[3]), False)
            cases[f"inv_{k}_tails{b}"] = (tab, signed(LOGIT_V if k == "logit" else PROBIT_V, d), True)
            if k == "logit":
                cases[f"inv_logit_clamped{b}"] = (tab, signed(LOGIT_V_CLAMPED, d), True)
    tab = table("periodic", d)
    cases["fwd_periodic"] = (tab, periodic_edge_x(tab[2], tab[3]), False)
    cases["inv_periodic"] = (tab, periodic_edge_x(tab[2], tab[3]), True)
    for k in ("affine", "logit_affine", "probit_affine"):
        tab = table(k, d)
        cases[f"fwd_{k}"] = (tab, interior_x(tab, 32, False, seed=5), False)
        cases[f"inv_{k}"] = (tab, interior_x(tab, 32, True, seed=5), True)
    for k in ("affine", "periodic", "logit", "probit", "logit_mix", "probit_mix"):
        tab = table(k, d)
        cases[f"fwd_{k}_nonfinite"] = (tab, poke_nonfinite(interior_x(tab, 70, False, seed=9)), False)
        cases[f"inv_{k}_nonfinite"] = (tab, poke_nonfinite(interior_x(tab, 70, True, seed=9)), True)
    return cases
