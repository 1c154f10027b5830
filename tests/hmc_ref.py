"""Host restatement of the random-walk and HMC mutations of the "blackjax_smc" sampler (include/asmc.h asmc_rw_* / asmc_mh_* /
asmc_hmc_*).

Philox draws go through stretch_ref's vectorised Philox4x32-10 (pinned to the oracle by tests/test_emcee_smc.py); on top of it: the
per-particle normal and accept streams, the mixture value and gradient, the random-walk proposal, the velocity-Verlet trajectory and
both accept rules, each written for any numpy float type - `np.longdouble` runs of the same code set the tolerances of the device
tests - and `HmcOracleEngine`, the CPU test double with the engine methods the sampler calls.  A test helper: the product never
imports it.
"""
from __future__ import annotations

import numpy as np
import torch

import stretch_ref as S
from oracle_engine import OracleEngine, _np

TAG_NORMAL = 0x20000000
TAG_ACCEPT = 0xFFFFFFFF
_TWO_M32 = 1.0 / 4294967296.0


def _key(seed):
    return int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF


def _gid_words(gid0, n):
    gid = np.uint64(gid0) + np.arange(n, dtype=np.uint64)
    return gid & np.uint64(0xFFFFFFFF), gid >> np.uint64(32)


def normals(seed, gid0, n, step, d):
    """xi [n, d]: coordinates 4 q .. 4 q + 3 of particle gid0 + i from the block {gid lo, gid hi, step, q | 0x20000000}; words
    (w0, w1) and (w2, w3) are (radius, angle) of two Box-Muller pairs on 32-bit uniforms (csrc/asmc_pcn_dev.h normal_quad), libm."""
    lo, hi = _gid_words(gid0, n)
    k0, k1 = _key(seed)
    nq = (d + 3) // 4
    out = np.empty((n, 4 * nq))
    for q in range(nq):
        w = S.philox4x32_10(lo, hi, step, q | TAG_NORMAL, k0, k1)
        for pair in (0, 1):
            u = (w[2 * pair].astype(np.float64) + 0.5) * _TWO_M32
            t = (w[2 * pair + 1].astype(np.float64) + 0.5) * _TWO_M32
            r = np.sqrt(-2.0 * np.log(u))
            out[:, 4 * q + 2 * pair] = r * np.cos(2.0 * np.pi * t)
            out[:, 4 * q + 2 * pair + 1] = r * np.sin(2.0 * np.pi * t)
    return out[:, :d]


def accept_uniforms(seed, gid0, n, step):
    lo, hi = _gid_words(gid0, n)
    k0, k1 = _key(seed)
    w = S.philox4x32_10(lo, hi, step, TAG_ACCEPT, k0, k1)
    return S.u01(w[0], w[1])


# ---- densities -------------------------------------------------------------------------------------------------------------------
def mix_value_grad(mix, x):
    """(log f(x) [n], grad log f(x) [n, d]) of a diagonal Gaussian mixture (logw, mu, prec) in x's float type."""
    ft = x.dtype
    logw, mu, prec = (np.asarray(a, dtype=ft) for a in mix)
    C = len(logw)
    terms = np.empty((x.shape[0], C), dtype=ft)
    for c in range(C):  # (component by component: no [n, C, d] temporaries)
        t = x - mu[c]
        terms[:, c] = logw[c] - ft.type(0.5) * (t * (prec[c] * t)).sum(-1)
    m = terms.max(axis=1)
    with np.errstate(all="ignore"):
        e = np.exp(terms - m[:, None])
        s = e.sum(axis=1)
        val = m + np.log(s)
        w = e / s[:, None]
        grad = np.zeros_like(x)
        for c in range(C):
            grad -= w[:, c, None] * (prec[c] * (x - mu[c]))
    return val, grad


def target(mixes, beta, x):
    """(ll, lp, lq, grad of (1 - beta) lq + beta (ll + lp)) at x."""
    ft = x.dtype.type
    (ll, gll), (lp, glp), (lq, glq) = (mix_value_grad(m, x) for m in mixes)
    return ll, lp, lq, ft(beta) * gll + ft(beta) * glp + ft(1.0 - beta) * glq


def log_p_t(ll, lp, lq, beta):
    ft = np.asarray(ll).dtype.type
    with np.errstate(all="ignore"):
        r = ft(1.0 - beta) * lq + ft(beta) * (ll + lp)
    return np.where(r < np.inf, r, -np.inf)


def kinetic(p, minv):
    return p.dtype.type(0.5) * ((p * p) if minv is None else (np.asarray(minv, dtype=p.dtype) * p * p)).sum(axis=1)


def leap(z, p, g, minv, kick, drift):
    """asmc_hmc_leap: p += kick g; z += drift minv p (returns new arrays)."""
    ft = z.dtype.type
    p = p + ft(kick) * g
    z = z + ft(drift) * (p if minv is None else np.asarray(minv, dtype=z.dtype) * p)
    return z, p


def trajectory(mixes, beta, x, p, g, eps, n_leap, minv):
    """n_leap velocity-Verlet steps from (x, p) with the gradient g at x: (x', p', ll', lp', lq', g')."""
    z, p = leap(x, p, g, minv, 0.5 * eps, eps)
    for i in range(n_leap):
        ll, lp, lq, g = target(mixes, beta, z)
        last = i == n_leap - 1
        z, p = leap(z, p, g, minv, 0.5 * eps if last else eps, 0.0 if last else eps)
    return z, p, ll, lp, lq, g


def momenta(seed, gid0, n, step, d, minv):
    xi = normals(seed, gid0, n, step, d)
    return xi if minv is None else xi / np.sqrt(np.asarray(minv, dtype=np.float64))


def hmc_transition(mixes, beta, x, eps, n_leap, minv, seed, gid0, step, ft=np.float64):
    """One HMC transition of every row in the float type `ft` (the momenta are the fp64 draws, widened): a dict with the end
    points, both energies and dH = [log p_t(x') - K(p')] - [log p_t(x) - K(p)]."""
    n, d = x.shape
    xf = x.astype(ft)
    p0 = momenta(seed, gid0, n, step, d, minv).astype(ft)
    ll0, lp0, lq0, g0 = target(mixes, beta, xf)
    z, p1, ll1, lp1, lq1, g1 = trajectory(mixes, beta, xf, p0, g0, eps, n_leap, minv)
    with np.errstate(all="ignore"):
        h0 = log_p_t(ll0, lp0, lq0, beta) - kinetic(p0, minv)
        h1 = log_p_t(ll1, lp1, lq1, beta) - kinetic(p1, minv)
        dH = h1 - h0
    return dict(x=z, p0=p0, p1=p1, new=(ll1, lp1, lq1), old=(ll0, lp0, lq0), g0=g0, g1=g1, h0=h0, h1=h1, dH=dH)


def hmc_decide(dH, seed, gid0, step):
    with np.errstate(all="ignore"):
        return np.log(accept_uniforms(seed, gid0, len(dH), step)) < np.asarray(dH, dtype=np.float64)


def hmc_mix(x, ll, lp, lq, beta, mixes, minv, eps, n_leap, seed, gid0, step0, n_steps):
    """asmc_hmc_mix in place on fp64 numpy arrays: (accept counts per transition, dH of the last transition)."""
    n = x.shape[0]
    counts = np.zeros(n_steps, dtype=np.int64)
    moved = np.zeros(n, dtype=bool)
    cur = target(mixes, beta, x)[:3]
    cur = [np.array(v) for v in cur]
    dH = np.zeros(n)
    for s in range(n_steps):
        r = hmc_transition(mixes, beta, x, eps, n_leap, minv, seed, gid0, step0 + s)
        dH = r["dH"]
        acc = hmc_decide(dH, seed, gid0, step0 + s)
        x[acc] = r["x"][acc]
        for c, v in zip(cur, r["new"]):
            c[acc] = v[acc]
        moved |= acc
        counts[s] = int(acc.sum())
    ll[moved], lp[moved], lq[moved] = cur[0][moved], cur[1][moved], cur[2][moved]
    return counts, dH


def random_mixture(g, C, d, spread=1.5):
    """(logw, mu, prec) of a C-component mixture with normalised components: means N(0, spread^2), variances in [0.5, 2]."""
    w = g.uniform(0.5, 1.5, size=C)
    var = g.uniform(0.5, 2.0, size=(C, d))
    logw = np.log(w / w.sum()) - 0.5 * d * np.log(2 * np.pi) - 0.5 * np.log(var).sum(axis=1)
    return logw, spread * g.normal(size=(C, d)), 1.0 / var


def dh_tolerance(mixes, beta, x, eps, n_leap, minv, seed, gid0, step):
    """The fp64 transition of the restatement and what a device may differ from it by: 8 x the largest distance between the fp64
    and the long-double run of this very case (another summation order, 1-ulp exp / log) plus 64 ulp of the row's larger energy;
    the same scheme for the end points, relative to the row's largest coordinate.  (r64, tol_dH [n], tol_x [n], gap)."""
    r64 = hmc_transition(mixes, beta, x, eps, n_leap, minv, seed, gid0, step)
    rld = hmc_transition(mixes, beta, x, eps, n_leap, minv, seed, gid0, step, ft=np.longdouble)
    ok = np.isfinite(r64["dH"]) & np.isfinite(rld["dH"].astype(np.float64))
    gap = float(np.max(np.abs(r64["dH"][ok] - rld["dH"][ok]).astype(np.float64))) if ok.any() else 0.0
    energy = np.maximum(np.abs(r64["h0"]), np.abs(r64["h1"]))
    tol_dH = 8.0 * gap + 64.0 * np.spacing(np.where(np.isfinite(energy), energy, 1.0))
    gap_x = float(np.max(np.abs(r64["x"] - rld["x"]).astype(np.float64)))
    tol_x = 8.0 * gap_x + 64.0 * np.spacing(np.abs(r64["x"]).max(axis=1))
    return r64, tol_dH, tol_x, gap


def split_fused_case(n=4097, d=7):
    """Inputs of the split-against-fused comparison: a three-component likelihood, a Gaussian prior and a Gaussian proposal as
    (mixes, x, beta, step_size, num_integration_steps, seed); `seed` is the key of a run's first mutation under rng_key = None."""
    from aspire_amd.samplers.blackjax_smc import mutation_seed
    from aspire_amd.targets import DiagGaussianMixture

    g = np.random.default_rng(4097)
    lik = DiagGaussianMixture(g.normal(size=(3, d)), g.uniform(0.5, 2.0, size=(3, d)), weights=[0.2, 0.3, 0.5])
    prior = DiagGaussianMixture(np.zeros((1, d)), 9.0)
    mu, sigma = 0.2 * g.normal(size=d), g.uniform(1.2, 1.8, size=d)
    lq = (np.array([-np.log(sigma).sum() - 0.5 * d * np.log(2 * np.pi)]), mu[None], (1.0 / sigma**2)[None])
    mixes = [(lik.logw, lik.mu, lik.prec), (prior.logw, prior.mu, prior.prec), lq]
    x = mu + sigma * g.normal(size=(n, d))
    return mixes, x, 0.6, 0.2, 5, mutation_seed(42, 0)


# ---- random walk -----------------------------------------------------------------------------------------------------------------
def rw_propose(x, sigma, seed, gid0, step):
    """asmc_rw_propose: sigma a float, a [d] array of standard deviations or a [d, d] lower-triangular factor; x's dtype."""
    n, d = x.shape
    xi = normals(seed, gid0, n, step, d)
    s = np.asarray(sigma, dtype=np.float64)
    inc = xi @ np.tril(s).T if s.ndim == 2 else s * xi
    return (x.astype(np.float64) + inc).astype(x.dtype)


def mh_accept(x, y, beta, ll, lp, lq, ll_new, lp_new, lq_new, seed, gid0, step, logj=None, logj_new=None):
    """asmc_mh_accept in place on numpy arrays; returns the decisions."""
    nlp, olp = S.log_p_t(ll_new, lp_new, lq_new, beta), S.log_p_t(ll, lp, lq, beta)
    with np.errstate(all="ignore"):
        if logj is not None:
            nlp, olp = nlp + logj_new, olp + logj
            nlp, olp = np.where(nlp < np.inf, nlp, -np.inf), np.where(olp < np.inf, olp, -np.inf)
        acc = nlp - olp > np.log(accept_uniforms(seed, gid0, x.shape[0], step))
    x[acc] = y[acc]
    ll[acc], lp[acc], lq[acc] = ll_new[acc], lp_new[acc], lq_new[acc]
    if logj is not None:
        logj[acc] = logj_new[acc]
    return acc


def hmc_accept(x, z_new, p0, p1, minv, beta, ll, lp, lq, ll_new, lp_new, lq_new, seed, gid0, step):
    """asmc_hmc_accept in place on numpy arrays; returns (decisions, dH)."""
    with np.errstate(all="ignore"):
        h0 = S.log_p_t(ll, lp, lq, beta) - kinetic(p0, minv)
        h1 = S.log_p_t(ll_new, lp_new, lq_new, beta) - kinetic(p1, minv)
        dH = h1 - h0
    acc = hmc_decide(dH, seed, gid0, step)
    x[acc] = z_new[acc].astype(x.dtype)
    ll[acc], lp[acc], lq[acc] = ll_new[acc], lp_new[acc], lq_new[acc]
    return acc, dH


class HmcOracleEngine(OracleEngine):
    """OracleEngine plus the random-walk / HMC entry points of HipEngine."""

    def __init__(self):
        super().__init__()
        self._mh_counts = np.zeros(2048, dtype=np.int64)

    @staticmethod
    def _mix(m):
        return (m.logw, m.mu, m.prec)

    def rw_propose(self, x, sigma, seed, gid0, step, t):
        self._mh_counts[t] = 0
        y = rw_propose(_np(x), _np(sigma) if isinstance(sigma, torch.Tensor) else sigma, seed, gid0, step)
        return torch.from_numpy(np.ascontiguousarray(y))

    def mh_accept(self, x, y, beta, ll, lp, lq, ll_new, lp_new, lq_new, seed, gid0, step, t, logj=None, logj_new=None):
        acc = mh_accept(x.numpy(), _np(y), beta, ll.numpy(), lp.numpy(), lq.numpy(), _np(ll_new).astype(np.float64),
                        _np(lp_new).astype(np.float64), _np(lq_new).astype(np.float64), seed, gid0, step,
                        None if logj is None else logj.numpy(), None if logj_new is None else _np(logj_new))
        self._mh_counts[t] += int(acc.sum())

    def mh_counts(self, n_steps):
        return self._mh_counts[:n_steps].copy()

    def hmc_momentum(self, n, d, minv, seed, gid0, step, t):
        self._mh_counts[t] = 0
        return torch.from_numpy(momenta(seed, gid0, n, step, d, None if minv is None else _np(minv)))

    def hmc_leap(self, z, p, g, minv, kick, drift):
        zn, pn = leap(z.numpy(), p.numpy(), _np(g), None if minv is None else _np(minv), kick, drift)
        z.copy_(torch.from_numpy(zn))
        p.copy_(torch.from_numpy(pn))

    def hmc_accept(self, x, z_new, p0, p1, minv, beta, ll, lp, lq, ll_new, lp_new, lq_new, seed, gid0, step, t, ke0=None, ke1=None,
                   want_dH=False):
        acc, dH = hmc_accept(x.numpy(), _np(z_new), _np(p0), _np(p1), None if minv is None else _np(minv), beta, ll.numpy(), lp.numpy(),
                             lq.numpy(), _np(ll_new).astype(np.float64), _np(lp_new).astype(np.float64),
                             _np(lq_new).astype(np.float64), seed, gid0, step)
        self._mh_counts[t] += int(acc.sum())
        return torch.from_numpy(acc), (torch.from_numpy(dH) if want_dH else None)

    def hmc_mix(self, x, ll, lp, lq, beta, t_ll, t_lp, t_lq, minv, step_size, n_leap, seed, gid0, step0, n_steps, t0=0, want_dH=False):
        assert x.dtype == torch.float64
        counts, dH = hmc_mix(x.numpy(), ll.numpy(), lp.numpy(), lq.numpy(), beta, [self._mix(m) for m in (t_ll, t_lp, t_lq)],
                             None if minv is None else _np(minv), step_size, n_leap, seed, gid0, step0, n_steps)
        self._mh_counts[t0:t0 + n_steps] = counts
        return torch.from_numpy(dH) if want_dH else None
