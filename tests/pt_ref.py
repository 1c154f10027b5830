"""CPU restatement of the parallel-tempering entry points (include/asmc.h asmc_pt_*): TEST INFRASTRUCTURE.

`swap_ref` is the replica exchange in numpy, its uniforms from `oracle.philox4x32_10` and the `u01` formula of tests/stretch_ref.py;
`evidence_table` restates the reductions of `asmc_pt_evidence`; `reference_ti` / `reference_stepping_stone` are a straight numpy
evaluation of the reference's formulas (samples.py:1013-1170) in any float type, the yardstick of the container's and the kernel's
tests.  `PTOracleEngine` is `ChainOracleEngine` (tests/chain_ref.py) plus `pt_swap` and `pt_evidence` - what the "pt_minipcn"
sampler asks of an engine beyond what "minipcn" does.  `gaussian_closed_form` and `pt_z_scores` are the statistical check the CPU
and the GPU sampler tests share.  The product never imports this file.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import oracle_engine as OE
from chain_ref import ChainOracleEngine
from stretch_ref import u01

O = OE.O
_np = OE._np

TAG_PT = 0x50000000


def swap_uniform(seed: int, rnd: int, r: int, w: int) -> float:
    """U(words 0, 1) of the block {w lo, w hi, round, 0x50000000 | r} under the key {seed lo, seed hi}."""
    words = O.philox4x32_10([w & 0xFFFFFFFF, (w >> 32) & 0xFFFFFFFF, rnd & 0xFFFFFFFF, TAG_PT | r],
                            [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
    return float(u01(int(words[0]), int(words[1])))


def swap_decisions(ll, betas, seed: int, rnd: int):
    """The pairs of round `rnd` and what decides them: (r of each pair [P], accept [P, W], log u [P, W], right-hand side [P, W])."""
    betas = np.asarray(betas, dtype=np.float64)
    T = betas.size
    ll = np.asarray(ll, dtype=np.float64).reshape(T, -1)
    W = ll.shape[1]
    rs = list(range(rnd & 1, T - 1, 2))
    if not rs:  # an odd round of two rungs, one rung: nobody meets
        return rs, np.zeros((0, W), dtype=bool), np.zeros((0, W)), np.zeros((0, W))
    logu = np.array([[math.log(swap_uniform(seed, rnd, r, w)) for w in range(W)] for r in rs]).reshape(len(rs), W)
    with np.errstate(invalid="ignore"):
        rhs = np.array([(betas[r] - betas[r + 1]) * (ll[r + 1] - ll[r]) for r in rs]).reshape(len(rs), W)
        ok = np.array([np.isfinite(ll[r]) & np.isfinite(ll[r + 1]) for r in rs]).reshape(len(rs), W)
        acc = ok & (logu < rhs)
    return rs, acc, logu, rhs


def swap_margin_ulps(ll, betas, seed: int, rnd: int) -> float:
    """Smallest distance between log u and the right-hand side over the decidable walkers, in ulps of the larger magnitude: a
    device log one ulp from numpy's can flip a decision only below 4."""
    rs, acc, logu, rhs = swap_decisions(ll, betas, seed, rnd)
    ok = np.isfinite(rhs)
    if not ok.any():
        return np.inf
    gap = np.abs(logu[ok] - rhs[ok]) / np.spacing(np.maximum(np.abs(logu[ok]), np.abs(rhs[ok])))
    return float(gap.min())


def swap_ref(x, ll, lp, betas, seed: int, rnd: int, companions=()):
    """One exchange round on copies: (x, ll, lp, companions, counts [T - 1]).  x [T W, d]; everything else [T W]."""
    T = len(betas)
    x, ll, lp = np.array(x, copy=True), np.array(ll, dtype=np.float64, copy=True), np.array(lp, dtype=np.float64, copy=True)
    comps = [np.array(c, dtype=np.float64, copy=True) for c in companions]
    W = ll.size // T
    counts = np.zeros(max(T - 1, 0), dtype=np.int64)
    rs, acc, _, _ = swap_decisions(ll, betas, seed, rnd)
    for p, r in enumerate(rs):
        a = r * W + np.flatnonzero(acc[p])
        b = a + W
        for v in (x, ll, lp, *comps):
            v[a], v[b] = v[b].copy(), v[a].copy()
        counts[r] = int(acc[p].sum())
    return x, ll, lp, comps, counts


def trapezoid_coefficients(betas):
    """coef [2, T] of asmc_pt_evidence for a descending ladder: the trapezoid's weight of every rung and the stepping-stone scale."""
    b = np.asarray(betas, dtype=np.float64)
    c, s = np.zeros(b.size), np.zeros(b.size)
    c[:-1] += 0.5 * (b[:-1] - b[1:])
    c[1:] += 0.5 * (b[:-1] - b[1:])
    s[1:] = b[:-1] - b[1:]
    return np.stack([c, s])


def evidence_table(ll, coef, ft=np.float64):
    """The [T + 1, 4] table of asmc_pt_evidence for kept samples ll [T, n], in float type `ft`."""
    ll = np.asarray(ll, dtype=ft)
    coef = np.asarray(coef, dtype=ft)
    T, n = ll.shape
    out = np.zeros((T + 1, 4), dtype=ft)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(T):
            a = coef[1, r] * ll[r]
            m = np.max(a)
            e = np.exp(a - m)
            out[r] = (np.sum(ll[r]), m, np.sum(e), np.sum(e * e))
        ti = np.zeros(n, dtype=ft)
        for r in range(T):
            ti = ti + coef[0, r] * ll[r]
        mean = np.mean(ti)
        out[T] = (n, mean, np.sum((ti - mean) ** 2), 0)
    return out


_trapezoid = getattr(np, "trapezoid", None) or np.trapz


def reference_ti(ll, betas, burn_in_fraction=0.1, method="variance", ft=np.float64):
    """samples.py:1045-1102 on ll [T, S, W] in float type `ft`: (log Z, error)."""
    ll = np.asarray(ll, dtype=ft)
    istart = int(ll.shape[1] * burn_in_fraction) if burn_in_fraction is not None else 0
    ll = ll[:, istart:].reshape(ll.shape[0], -1)
    order = np.argsort(betas)
    b, y = np.asarray(betas, dtype=ft)[order], ll[order]
    with np.errstate(invalid="ignore", over="ignore"):
        means = np.mean(y, axis=1)
        logz = _trapezoid(means, b)
        if method == "variance":
            ti = _trapezoid(y, b, axis=0)
            return logz, np.sqrt(np.var(ti) / ft(ti.shape[0]))
        b, m = b[::-1], means[::-1]
        if b[-1] != 0:
            b2, m2 = np.concatenate((b[::2], [0])), np.concatenate((m[::2], [m[-1]]))
        else:
            b2, m2 = np.concatenate((b[:-1:2], [0])), np.concatenate((m[:-1:2], [m[-1]]))
        return logz, abs(logz - (-_trapezoid(m2, b2)))


def reference_stepping_stone(ll, betas, burn_in_fraction=0.1, ft=np.float64):
    """samples.py:1128-1170 on ll [T, S, W] in float type `ft`: (log Z, error)."""
    ll = np.asarray(ll, dtype=ft)
    istart = int(ll.shape[1] * burn_in_fraction) if burn_in_fraction is not None else 0
    ll = ll[:, istart:].reshape(ll.shape[0], -1)
    order = np.argsort(betas)[::-1]
    b, y = np.asarray(betas, dtype=ft)[order], ll[order]
    logz, var, n = ft(0), ft(0), y.shape[1]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j in range(len(b) - 1):
            a = (b[j] - b[j + 1]) * y[j + 1]
            a_max = np.max(a)
            shifted = np.exp(a - a_max)
            mean_shift = np.mean(shifted)
            logz = logz + np.log(mean_shift) + a_max
            var = var + np.sum((shifted / mean_shift) ** 2)
        return logz, np.sqrt(var / ft(n) ** 2)


class PTOracleEngine(ChainOracleEngine):
    def pt_swap(self, x, ll, lp, betas, seed, rnd, counts, c0=None, c1=None):
        comps = [c for c in (c0, c1) if c is not None]
        xo, llo, lpo, co, cnt = swap_ref(_np(x), _np(ll), _np(lp), _np(betas), int(seed), int(rnd), [_np(c) for c in comps])
        x.copy_(torch.from_numpy(xo))
        ll.copy_(torch.from_numpy(llo))
        lp.copy_(torch.from_numpy(lpo))
        for c, v in zip(comps, co):
            c.copy_(torch.from_numpy(v))
        if counts is not None and cnt.size:
            counts[:cnt.size] += torch.from_numpy(cnt)

    def pt_evidence(self, ll, n_temps, stride, offset, n, coef):
        rows = _np(ll).reshape(n_temps, stride)[:, offset:offset + n]
        return evidence_table(rows, np.asarray(coef, dtype=np.float64).reshape(2, n_temps))


# ---- the Gaussian case of the statistical check: prior N(0, sp2 I), likelihood N(x; m, sl2 I), both normalised --------------------
def gaussian_closed_form(m, sp2: float, sl2: float, betas):
    """(mean log-likelihood of every rung [T], log Z)."""
    m = np.asarray(m, dtype=np.float64)
    d = m.size
    means = []
    for b in np.asarray(betas, dtype=np.float64):
        lam = 1.0 / sp2 + b / sl2
        mu = (b / sl2) * m / lam
        means.append(-0.5 * d * math.log(2 * math.pi * sl2) - (d / lam + float(np.sum((mu - m) ** 2))) / (2 * sl2))
    s2 = sp2 + sl2
    logz = -0.5 * d * math.log(2 * math.pi * s2) - float(np.sum(m**2)) / (2 * s2)
    return np.array(means), logz


def pt_z_scores(ll, betas, mean_ll, logz):
    """z-scores of a run's kept log-likelihoods ll [T, S, W] against the closed form, with standard errors from the between-walker
    spread of the run itself (as chain_ref.moment_z_scores): column w of every rung - walker w meets only walker w - is one of W
    systems of the same law, so with f_w a statistic's value on column w alone, se = std(f_w) / sqrt(W).
      rung means   f_w = time average of ll[r, :, w]
      TI           f_w = trapezoid over beta of column w's time averages (linear: their mean is the pooled estimate); the target is
                   the trapezoid of the closed-form means on the same ladder
      stepping stone  log Z = sum_j log r_j with r_j the pooled mean of exp(dbeta_j ll[j + 1]); linearised, f_w = sum_j r_jw / r_j
    Returns (z of the rung means [T], z of TI, z of the stepping stone)."""
    ll = np.asarray(ll, dtype=np.float64)
    betas = np.asarray(betas, dtype=np.float64)
    T, S, W = ll.shape
    col = ll.mean(axis=1)  # [T, W]
    z_mean = (col.mean(axis=1) - mean_ll) / (col.std(axis=1, ddof=1) / math.sqrt(W))
    order = np.argsort(betas)
    ti_w = _trapezoid(col[order], betas[order], axis=0)
    z_ti = (ti_w.mean() - _trapezoid(np.asarray(mean_ll)[order], betas[order])) / (ti_w.std(ddof=1) / math.sqrt(W))
    log_ss, g = 0.0, np.zeros(W)
    for j in range(T - 1):
        a = (betas[j] - betas[j + 1]) * ll[j + 1]
        a_max = a.max()
        e = np.exp(a - a_max)
        r = e.mean()
        log_ss += math.log(r) + a_max
        g += e.mean(axis=0) / r
    z_ss = (log_ss - logz) / (g.std(ddof=1) / math.sqrt(W))
    return z_mean, z_ti, z_ss


GAUSS_D = 4
GAUSS_M = np.array([1.0, -0.5, 0.5, 1.5])
GAUSS_SP2, GAUSS_SL2 = 4.0, 0.25


def gaussian_targets():
    """(likelihood N(x; m, 0.25 I), prior N(0, 4 I)) at d = 4 as normalised built-in mixtures."""
    from aspire_amd.targets import DiagGaussianMixture

    return (DiagGaussianMixture(GAUSS_M[None, :], GAUSS_SL2, normalized=True),
            DiagGaussianMixture(np.zeros((1, GAUSS_D)), GAUSS_SP2, normalized=True))
