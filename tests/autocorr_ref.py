"""Numpy restatement of the chain diagnostics (include/asmc.h asmc_chain_series_moments / _acf_* / _rhat) by DIRECT SUMMATION in fp64:
TEST INFRASTRUCTURE, written from the formulas of DESIGN.md section 3.23, not from the kernels.

    rho_j[k] = (1 / W) sum_w ( sum_{t = 0}^{S - 1 - k} (x_t - m)(x_{t+k} - m) ) / c0,   m, c0 per series
    tau_k    = 2 sum_{i <= k} rho_j[i] - 1,   window = first k with not (k < c tau_k), else S - 1
    A_j[k]   = (1 / W) sum_w sum_t |(x_t - m)(x_{t+k} - m)| / c0     (<= 1 by Cauchy-Schwarz: the mass the tolerance scales with)

`DiagOracleEngine` is `ChainOracleEngine` (tests/chain_ref.py) plus `chain_autocorr` / `chain_rhat` from these functions (`DiagMixin`
puts them on any other test double), so the container- and sampler-level tests run without a GPU.  `fixture` / `GPU_SHAPES` are
the chains that tests/test_gpu_chain_diagnostics.py runs and tests/test_chain_diagnostics.py guards against razor-edge windows.
"""
from __future__ import annotations

import numpy as np

from chain_ref import ChainOracleEngine

U = 2.0 ** -53
KB = 32  # ASMC_DIAG_KB: the GPU test checks that the binding says the same
PHIS = (0.0, 0.5, 0.9, 0.3, 0.8)  # coordinate j of a fixture is AR(1) with PHIS[j % 5]: the coordinates finish in different lag blocks
GPU_SHAPES = [(S, W, d) for S in (1, 2, KB - 1, KB, KB + 1, 2 * KB + 3, 131) for W in (1, 7, 257) for d in (1, 3, 8, 32, 33)]


def gamma(n: int) -> float:
    """Higham's gamma_n = n u / (1 - n u): bounds the relative error of a sum of n fp64 terms, in any order."""
    return n * U / (1.0 - n * U)


def rho_bound(S: int, W: int, mass):
    """|rho_a - rho_b| <= 8 gamma_{S W} A for two fp64 evaluations that differ in the order of their sums."""
    return 8.0 * gamma(S * W) * np.asarray(mass)


def ar1(seed: int, S: int, W: int, phi, dtype=np.float64) -> np.ndarray:
    """A stationary AR(1) ensemble [S, W, d] with zero mean, unit variance and per-coordinate coefficient phi [d]."""
    phi = np.atleast_1d(np.asarray(phi, dtype=np.float64))
    g = np.random.default_rng(seed)
    x = np.empty((S, W, phi.size))
    x[0] = g.normal(size=(W, phi.size))
    for t in range(1, S):
        x[t] = phi * x[t - 1] + np.sqrt(1.0 - phi**2) * g.normal(size=(W, phi.size))
    return x.astype(dtype)


def fixture(S: int, W: int, d: int, dtype=np.float64, seed: int = 0) -> np.ndarray:
    """The chain of shape case (S, W, d): mixed phi per coordinate, seeded by the shape."""
    return ar1(1000 * seed + 7919 * S + 31 * W + d, S, W, [PHIS[j % len(PHIS)] for j in range(d)], dtype)


def special_fixtures():
    """The special cases of tests/test_gpu_chain_diagnostics.py."""
    out = {"short-0.99": ar1(13, 50, 7, [0.99, 0.5, 0.99])}
    x = fixture(40, 9, 5)
    x[:, :, 2] = -1.25
    out["constant-coordinate"] = x
    x = fixture(40, 9, 5)
    x[:, 4, 1] = 0.5
    out["constant-walker"] = x
    out["guarded"] = fixture(37, 11, 6)
    out["rungs"] = np.stack([fixture(29, 13, 4, seed=s) for s in (1, 2, 3)])
    return out


def autocorr_direct(chain, c: float = 5.0, all_lags: bool = False):
    """dict(rho, mass, taus [S, d], window [d], tau [d]) of a chain [S, W, d].  Lags are evaluated until every coordinate has its
    window (all of them with `all_lags`); rows behind that are NaN."""
    x = np.asarray(chain, dtype=np.float64)
    S, W, d = x.shape
    y = x - np.sum(x, axis=0) / S
    c0 = np.sum(y * y, axis=0)  # [W, d]
    rho, mass, taus = (np.full((S, d), np.nan) for _ in range(3))
    window, done, run = np.full(d, S - 1, dtype=np.int64), np.zeros(d, dtype=bool), np.zeros(d)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(S):
            p = y[:S - k] * y[k:]
            rho[k] = np.sum(np.sum(p, axis=0) / c0, axis=0) / W
            mass[k] = np.sum(np.sum(np.abs(p), axis=0) / c0, axis=0) / W
            run = run + rho[k]
            taus[k] = 2.0 * run - 1.0
            hit = ~done & ~(k < c * taus[k])
            window[hit & ~np.isnan(taus[k])] = k  # (NaN: no window, the last lag - whose tau is NaN too)
            done |= hit
            if done.all() and not all_lags:
                break
    tau = np.where(np.isnan(taus[0]), np.nan, taus[window, np.arange(d)])
    return dict(rho=rho, mass=mass, taus=taus, window=window, tau=tau)


def razor_margin(chain, c: float = 5.0) -> float:
    """min over coordinates and lags up to the window of |k - c tau_k|: how far every window decision is from flipping."""
    r = autocorr_direct(chain, c)
    worst = np.inf
    for j, w in enumerate(r["window"]):
        t = r["taus"][:w + 1, j]
        if not np.isnan(t).any():
            worst = min(worst, float(np.min(np.abs(np.arange(w + 1) - c * t))))
    return worst


def split_rhat_direct(chain):
    """(rhat [d], kappa [d]) of a chain [S, W, d]: split R-hat, and the ratio of absolute mass to value of the one sum in it that
    cancels, kappa = sum_c |dev_c| (a_c + mean_c a_c) / sum_c dev_c^2 with dev_c the half-chain's mean minus the grand mean and a_c
    its mean absolute value (the other sums add non-negative terms)."""
    x = np.asarray(chain, dtype=np.float64)
    S, W, d = x.shape
    n = S // 2
    if n < 2:
        return np.full(d, np.nan), np.full(d, np.nan)
    means, var, absm = [], [], []
    for half in (x[:n], x[S - n:]):
        m = np.sum(half, axis=0) / n
        means.append(m)
        var.append(np.sum((half - m) ** 2, axis=0) / (n - 1))
        absm.append(np.sum(np.abs(half), axis=0) / n)
    means, var, absm = np.concatenate(means), np.concatenate(var), np.concatenate(absm)  # [2 W, d]
    M = 2 * W
    dev = means - np.sum(means, axis=0) / M
    ssd = np.sum(dev**2, axis=0)
    Wv = np.sum(var, axis=0) / M
    with np.errstate(invalid="ignore", divide="ignore"):
        rhat = np.sqrt(((n - 1) / n * Wv + n / (M - 1) * ssd / n) / Wv)
        kappa = np.sum(np.abs(dev) * (absm + np.sum(absm, axis=0) / M), axis=0) / ssd
    return rhat, kappa


class DiagMixin:
    """`HipEngine.chain_autocorr` / `chain_rhat` on host tensors (same signatures)."""

    def chain_autocorr(self, chain_x, c: float = 5.0, return_rho: bool = False, kb=None):
        assert chain_x.dim() == 3 and chain_x.is_contiguous()
        r = autocorr_direct(chain_x.numpy(), c)
        if not return_rho:
            return r["tau"], r["window"]
        rho = r["rho"].T.copy()
        for j, w in enumerate(r["window"]):
            rho[j, w + 1:] = np.nan
        return r["tau"], r["window"], rho

    def chain_rhat(self, chain_x):
        assert chain_x.dim() == 3 and chain_x.is_contiguous()
        return split_rhat_direct(chain_x.numpy())[0]


class DiagOracleEngine(DiagMixin, ChainOracleEngine):
    pass
