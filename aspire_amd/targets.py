"""Built-in device-resident log-densities for `log_likelihood` / `log_prior`.

The reference takes arbitrary Python callables `f(samples) -> array` (src/aspire/samplers/base.py:81-91).
Those still work here (split propose/accept path), but a callable that is an instance of
`DiagGaussianMixture` is *recognised* by the sampler and evaluated inside the fused pCN kernel, so
the particle state never leaves HBM.  `GaussianMixture` (full covariances, box bounds) is
recognised on the un-fused paths and evaluated by its own kernel, value and gradient in one launch.  Called directly it behaves like any other
user callable and evaluates the same formula with plain array ops of the samples' namespace.
"""
from __future__ import annotations

import logging
import math

import numpy as np
import torch

from ._xp import is_torch


class DiagGaussianMixture:
    """log sum_c w_c N(x; mean_c, diag var_c)  (or the un-normalised form).

    Parameters
    ----------
    means : [C, d] or [d]
    variances : [C, d], [d] or scalar
    weights : [C] mixture weights (default equal)
    normalized : include the -d/2 log(2 pi) - 1/2 sum log var terms (default True)
    log_scale : constant added to the log-density
    """

    def __init__(self, means, variances=1.0, weights=None, normalized: bool = True, log_scale: float = 0.0):
        mu = np.atleast_2d(np.asarray(means, dtype=np.float64))
        C, d = mu.shape
        var = np.broadcast_to(np.asarray(variances, dtype=np.float64), (C, d)).copy()
        if np.any(var <= 0):
            raise ValueError("variances must be positive")
        w = np.full(C, 1.0 / C) if weights is None else np.asarray(weights, dtype=np.float64)
        if w.shape != (C,) or np.any(w <= 0):
            raise ValueError("weights must be C positive numbers")
        self.mu, self.prec = mu, 1.0 / var
        logw = np.log(w / w.sum()) + log_scale
        if normalized:
            logw = logw - 0.5 * d * math.log(2 * math.pi) - 0.5 * np.sum(np.log(var), axis=1)
        self.logw = logw
        self.dims = d
        self._dev = {}

    @classmethod
    def isotropic(cls, dims: int, mean: float = 0.0, var: float = 1.0, normalized: bool = True):
        return cls(np.full((1, dims), mean), var, normalized=normalized)

    def device_mixture(self, engine):
        key = id(engine)
        if key not in self._dev:
            self._dev[key] = engine.make_mixture(self.logw, self.mu, self.prec)
        return self._dev[key]

    def __call__(self, samples):
        x = samples.x if hasattr(samples, "x") else samples
        if is_torch(x):
            mu = torch.as_tensor(self.mu, dtype=torch.float64, device=x.device)
            pr = torch.as_tensor(self.prec, dtype=torch.float64, device=x.device)
            lw = torch.as_tensor(self.logw, dtype=torch.float64, device=x.device)
            t = x.to(torch.float64)[:, None, :] - mu[None]
            terms = lw[None] - 0.5 * (t * t * pr[None]).sum(-1)
            return terms[:, 0] if terms.shape[1] == 1 else torch.logsumexp(terms, dim=1)
        x = np.asarray(x, dtype=np.float64)
        t = x[:, None, :] - self.mu[None]
        terms = self.logw[None] - 0.5 * (t * t * self.prec[None]).sum(-1)
        if terms.shape[1] == 1:
            return terms[:, 0]
        m = terms.max(axis=1)
        with np.errstate(invalid="ignore"):
            out = m + np.log(np.exp(terms - m[:, None]).sum(axis=1))
        return np.where(np.isneginf(m), -np.inf, out)


logger = logging.getLogger(__name__)

MAX_COMPONENTS = 8  # ASMC_MAX_COMPONENTS
KERNEL_MAX_DIMS = 128  # widest row asmc_fullmix_logpdf takes
KERNEL_GRAD_MAX_DIMS = 64  # widest row whose gradient the kernel returns faster than torch.autograd on __call__


def _lower_factor_from_precision(P: np.ndarray) -> tuple[np.ndarray, bool]:
    """(W, singular): lower-triangular W with W^T W = P for a symmetric positive SEMI-definite P, in fp64, by a route that
    always exists: eigendecomposition P = V diag(lam) V^T, S = diag(sqrt(lam)) V^T (S^T S = P), then the QR factorisation of S
    with its columns reversed, S J = Q R: W = J R J is lower-triangular and W^T W = J R^T R J = S^T S."""
    d = P.shape[0]
    if not np.all(np.isfinite(P)) or not np.allclose(P, P.T, rtol=1e-10, atol=1e-12 * max(1.0, float(np.abs(P).max()))):
        raise ValueError("a precision matrix must be finite and symmetric")
    lam, V = np.linalg.eigh(0.5 * (P + P.T))
    top = max(float(lam.max()), 0.0)
    if lam.min() < -64.0 * d * np.finfo(np.float64).eps * max(top, np.finfo(np.float64).tiny):
        raise ValueError("a precision matrix must be positive semi-definite")
    singular = bool(lam.min() <= 64.0 * d * np.finfo(np.float64).eps * top)
    S = np.sqrt(np.clip(lam, 0.0, None))[:, None] * V.T
    R = np.linalg.qr(S[:, ::-1], mode="r")
    W = np.tril(R[::-1, ::-1])
    sign = np.where(np.diag(W) < 0.0, -1.0, 1.0)
    return W * sign[:, None], singular


class _FullMixFunction(torch.autograd.Function):
    """value and per-row gradient from ONE launch; backward is grad_out[:, None] * G."""

    @staticmethod
    def forward(ctx, x, target, engine):
        out, G = engine.fullmix_logpdf(x.detach(), target.device_tables(engine), want_grad=True)
        ctx.save_for_backward(G)
        ctx.x_dtype = x.dtype
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (G,) = ctx.saved_tensors
        return (grad_out[:, None] * G).to(ctx.x_dtype), None, None


class GaussianMixture:
    """log sum_c exp(logw_c - 1/2 |W_c (x - mu_c)|^2) inside an optional closed box: full covariances, bounded support.

    W_c is lower-triangular with W_c^T W_c = P_c, the precision of component c (attribute `whiten`).

    Parameters
    ----------
    means : [C, d] or [d]
    covariances : [C, d, d], or [d, d] shared by every component; symmetric positive definite (W = inv(cholesky))
    precisions : the same shapes, given INSTEAD of covariances; symmetric positive SEMI-definite is allowed (a zero matrix is a
        flat component; the precision of a linear model with fewer data than parameters is singular)
    weights : [C] mixture weights (default equal)
    bounds : (lower, upper), each [d] or a scalar.  The box is closed.  A row with a finite coordinate outside
        [lower_j, upper_j] has log-density -inf.  The mixture is NOT renormalised for the truncation: inside the box the density
        is the unbounded mixture's, so it integrates to the mixture's mass inside the box, not to one
    normalized : add -(d/2) log(2 pi) + sum log diag(W_c) (default True); a singular precision has no such constant and raises
        ValueError - say normalized=False
    log_scale : constant added to the log-density

    Non-finite rows: a NaN coordinate gives NaN (before the bounds are looked at); a +-inf coordinate and no NaN gives -inf.

    Called directly it evaluates the formula with plain array ops of the samples' namespace (differentiable on torch tensors) and
    launches no kernel; `evaluate(engine, x)` is the HIP kernel (asmc_fullmix_logpdf), which the samplers use.
    """

    def __init__(self, means, covariances=None, *, precisions=None, weights=None, bounds=None, normalized: bool = True,
                 log_scale: float = 0.0):
        mu = np.atleast_2d(np.asarray(means, dtype=np.float64))
        if mu.ndim != 2:
            raise ValueError("means must be [C, d] or [d]")
        C, d = mu.shape
        if C > MAX_COMPONENTS:
            raise ValueError(f"at most {MAX_COMPONENTS} components")
        if (covariances is None) == (precisions is None):
            raise ValueError("pass exactly one of covariances and precisions")
        M = np.asarray(covariances if precisions is None else precisions, dtype=np.float64)
        if M.shape == (d, d):
            M = np.broadcast_to(M, (C, d, d))
        if M.shape != (C, d, d):
            raise ValueError(f"matrices must be [{C}, {d}, {d}] or [{d}, {d}], got {M.shape}")
        W = np.zeros((C, d, d))
        singular = False
        for c in range(C):
            if precisions is None:
                if not np.all(np.isfinite(M[c])) or not np.allclose(M[c], M[c].T, rtol=1e-10, atol=1e-12 * max(1.0, float(np.abs(M[c]).max()))):
                    raise ValueError("a covariance matrix must be symmetric positive definite")
                try:
                    L = np.linalg.cholesky(0.5 * (M[c] + M[c].T))
                except np.linalg.LinAlgError as e:
                    raise ValueError("a covariance matrix must be symmetric positive definite") from e
                W[c] = np.tril(np.linalg.solve(L, np.eye(d)))
            else:
                W[c], s = _lower_factor_from_precision(M[c])
                singular = singular or s
        w = np.full(C, 1.0 / C) if weights is None else np.asarray(weights, dtype=np.float64)
        if w.shape != (C,) or np.any(~(w > 0)):
            raise ValueError("weights must be C positive numbers")
        logw = np.log(w / w.sum()) + float(log_scale)
        if normalized:
            if singular:
                raise ValueError("a singular precision has no normalising constant: pass normalized=False")
            logw = logw - 0.5 * d * math.log(2 * math.pi) + np.sum(np.log(np.diagonal(W, axis1=1, axis2=2)), axis=1)
        self.lower = self.upper = None
        if bounds is not None:
            lo, hi = bounds
            lo = np.broadcast_to(np.asarray(lo, dtype=np.float64), (d,)).copy()
            hi = np.broadcast_to(np.asarray(hi, dtype=np.float64), (d,)).copy()
            if np.any(np.isnan(lo)) or np.any(np.isnan(hi)) or np.any(lo > hi):
                raise ValueError("bounds must satisfy lower <= upper")
            self.lower, self.upper = lo, hi
        self.mu, self.whiten, self.logw = mu, W, logw
        self.dims, self.n_components = d, C
        self._dev = {}
        self._fallback_logged = False
        self._wide_grad_logged = False

    @classmethod
    def uniform(cls, lower, upper):
        """The normalised uniform density on the closed box [lower, upper]: one flat component, logw = -sum log(upper - lower)."""
        lo, hi = np.atleast_1d(np.asarray(lower, dtype=np.float64)), np.atleast_1d(np.asarray(upper, dtype=np.float64))
        lo, hi = np.broadcast_arrays(lo, hi)
        if not np.all(np.isfinite(lo)) or not np.all(np.isfinite(hi)) or np.any(hi <= lo):
            raise ValueError("uniform needs finite lower < upper")
        d = lo.shape[0]
        return cls(0.5 * (lo + hi), precisions=np.zeros((d, d)), bounds=(lo, hi), normalized=False,
                   log_scale=-float(np.sum(np.log(hi - lo))))

    @classmethod
    def from_linear_model(cls, A, y, sigma, normalized: bool = True):
        """One component equal to -1/2 sum_k ((y_k - (A x)_k) / sigma_k)^2 (A [m, d], y [m], sigma a scalar or [m]; any m, also
        m < d: the precision is then singular).  normalized=True also subtracts sum_k log(sigma_k sqrt(2 pi)).  The residual of
        the least-squares fit goes into logw."""
        A = np.atleast_2d(np.asarray(A, dtype=np.float64))
        y = np.atleast_1d(np.asarray(y, dtype=np.float64))
        m, d = A.shape
        sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (m,))
        if y.shape != (m,) or np.any(~(sig > 0)):
            raise ValueError("from_linear_model: A [m, d], y [m], sigma positive")
        As, ys = A / sig[:, None], y / sig
        mean = np.linalg.lstsq(As, ys, rcond=None)[0]
        res = ys - As @ mean
        log_scale = -0.5 * float(res @ res)
        if normalized:
            log_scale -= float(np.sum(np.log(sig))) + 0.5 * m * math.log(2 * math.pi)
        return cls(mean, precisions=As.T @ As, normalized=False, log_scale=log_scale)

    def device_tables(self, engine):
        key = id(engine)
        if key not in self._dev:
            self._dev[key] = engine.make_fullmix(self.logw, self.mu, self.whiten, self.lower, self.upper)
        return self._dev[key]

    def evaluate(self, engine, x, grad: bool = False):
        """fp64 [n] log-density of the rows x from the HIP kernel; grad=True: (value, gradient [n, d]) from the same launch.  On a
        tensor that requires grad the value carries its gradient through torch.autograd.  A shape the kernel refuses - or an
        engine without it, or a gradient at more than 64 dimensions (where the kernel measured slower than the array ops) - is
        evaluated by `__call__`."""
        ok = (hasattr(engine, "fullmix_logpdf") and is_torch(x) and x.dim() == 2 and x.is_cuda and x.shape[0] > 0
              and x.dtype in (torch.float64, torch.float32) and x.shape[1] == self.dims and self.dims <= KERNEL_MAX_DIMS)
        if ok and self.dims > KERNEL_GRAD_MAX_DIMS and (grad or (x.requires_grad and torch.is_grad_enabled())):
            ok = False  # measured: at d = 128 the kernel's gradient sweep is slower than autograd through the array ops
            if not self._wide_grad_logged:
                self._wide_grad_logged = True
                logger.info("GaussianMixture: gradients above %d dimensions are taken by autograd through the array ops "
                            "(faster than the kernel's gradient sweep there)", KERNEL_GRAD_MAX_DIMS)
        elif not ok and not self._fallback_logged:
            self._fallback_logged = True
            logger.info("GaussianMixture: no kernel for this engine / shape; evaluating with array ops")
        if not ok:
            if not grad:
                return self(x)
            with torch.enable_grad():
                leaf = torch.as_tensor(x).detach().clone().requires_grad_(True)
                val = self(leaf)
                g = torch.autograd.grad(torch.where(torch.isfinite(val), val, torch.zeros_like(val)).sum(), leaf)[0]
            return val.detach(), g.to(torch.float64)
        xc = x if x.is_contiguous() else x.contiguous()
        if grad:
            return engine.fullmix_logpdf(xc.detach(), self.device_tables(engine), want_grad=True)
        if xc.requires_grad and torch.is_grad_enabled():
            return _FullMixFunction.apply(xc, self, engine)
        return engine.fullmix_logpdf(xc.detach(), self.device_tables(engine))

    def __call__(self, samples):
        x = samples.x if hasattr(samples, "x") else samples
        if is_torch(x):
            kw = dict(dtype=torch.float64, device=x.device)
            mu, W, lw = (torch.as_tensor(a, **kw) for a in (self.mu, self.whiten, self.logw))
            x = x.to(torch.float64)
            nan_row = torch.isnan(x).any(dim=1)
            bad = torch.isinf(x).any(dim=1)
            if self.lower is not None:
                lo, hi = torch.as_tensor(self.lower, **kw), torch.as_tensor(self.upper, **kw)
                bad = bad | ((x < lo) | (x > hi)).any(dim=1)
            plain = ~(nan_row | bad)
            r = torch.where(plain[:, None], x, torch.zeros_like(x))[:, None, :] - mu[None]
            v = torch.einsum("cij,ncj->nci", W, r)
            q = (v * v).sum(-1)
            q = torch.where(torch.isnan(q), torch.full_like(q, math.inf), q)  # products overflowed: the row is too far
            terms = lw[None] - 0.5 * q
            if terms.shape[1] == 1:
                out = terms[:, 0]
            else:
                far = torch.isneginf(terms.max(dim=1).values)
                out = torch.logsumexp(torch.where(far[:, None], torch.zeros_like(terms), terms), dim=1)
                out = torch.where(far, torch.full_like(out, -math.inf), out)
            out = torch.where(bad, torch.full_like(out, -math.inf), out)
            return torch.where(nan_row, torch.full_like(out, math.nan), out)
        x = np.asarray(x, dtype=np.float64)
        nan_row = np.isnan(x).any(axis=1)
        bad = np.isinf(x).any(axis=1)
        if self.lower is not None:
            with np.errstate(invalid="ignore"):
                bad = bad | ((x < self.lower) | (x > self.upper)).any(axis=1)
        plain = ~(nan_row | bad)
        r = np.where(plain[:, None], x, 0.0)[:, None, :] - self.mu[None]
        with np.errstate(over="ignore", invalid="ignore"):
            v = np.einsum("cij,ncj->nci", self.whiten, r)
            q = (v * v).sum(-1)
            q = np.where(np.isnan(q), np.inf, q)
            terms = self.logw[None] - 0.5 * q
            if terms.shape[1] == 1:
                out = terms[:, 0].copy()
            else:
                m = terms.max(axis=1)
                out = m + np.log(np.exp(terms - m[:, None]).sum(axis=1))
                out = np.where(np.isneginf(m), -np.inf, out)
        out = np.where(bad, -np.inf, out)
        return np.where(nan_row, np.nan, out)
