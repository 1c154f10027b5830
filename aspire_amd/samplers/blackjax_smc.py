"""The `"blackjax_smc"` sampler: the SMC loop of `SMCSampler` with random-walk Metropolis-Hastings, Hamiltonian Monte Carlo or NUTS as
the mutation.

`HipBlackJAXSMC` mirrors reference src/aspire/samplers/smc/blackjax.py:13-349.  Every particle is an independent chain on the tempered
log-target (smc/base.py:507-519); the transitions are this repository's HIP kernels (csrc/asmc_hmc.hip, csrc/asmc_nuts.hip) instead of
the third-party `blackjax` and `jax` packages, which are absent: parity with their random streams is unpinned (DESIGN.md §3.13,
§3.18).  The default algorithm here is `"hmc"`; the reference's default `"nuts"` runs on request.
"""
from __future__ import annotations

import logging
import math

import numpy as np
import torch

from .._xp import is_torch_namespace
from ..flows import GaussianFlow
from ..targets import DiagGaussianMixture, GaussianMixture
from .base import track_calls
from .smc import DEFAULT_BETA_TOLERANCE, SMCSampler

logger = logging.getLogger(__name__)

MAX_CHUNK = 2048  # steps whose accept counts the device holds (ASMC_MAX_PCN_STEPS): one read-back per chunk
NUTS_MAX_LAUNCH = 256  # transitions of one fused NUTS launch (k_nuts_mix keeps their statistics in LDS)
NUTS_MAX_DOUBLINGS = 10  # ASMC_NUTS_MAX_DOUBLINGS
FUSED_MAX_DIMS = 128  # k_hmc_mix keeps a row of up to 128 coordinates in registers
FUSED_MAX_COMPONENTS = 8  # ASMC_MAX_COMPONENTS
SAMPLER_KWARGS = ("n_steps", "algorithm", "step_size", "num_integration_steps", "inverse_mass_matrix", "sigma", "n_final_steps",
                  "flow_sample_on_engine", "max_num_doublings", "divergence_threshold")
RW_ALGORITHMS = ("rwmh", "random_walk")
_default_logged = False


def mutation_seed(seed: int, m: int) -> int:
    """Philox key of mutation `m` of a run seeded with `seed`."""
    return int(np.random.SeedSequence([int(seed), int(m)]).generate_state(1, np.uint64)[0])


def proposal_scale(sigma, dims: int):
    """`sigma` of the random-walk proposal as (mode, value): a scalar or a 1-D array are standard deviations (blackjax.py:171-189),
    a 2-D array is a covariance, handed on as its lower Cholesky factor (fp64, host).  The reference tells the two array forms apart
    by `len(sigma) == dims`, which sends a [d, d] covariance down its diagonal branch; here the number of axes decides."""
    s = np.asarray(sigma.detach().cpu() if isinstance(sigma, torch.Tensor) else sigma, dtype=np.float64)
    if s.ndim == 0:
        if not (np.isfinite(s) and s > 0):
            raise ValueError(f"sigma must be positive and finite, got {float(s)}")
        return "scalar", float(s)
    if s.ndim == 1:
        if s.shape != (dims,) or not np.all(np.isfinite(s) & (s > 0)):
            raise ValueError(f"a 1-D sigma holds {dims} positive standard deviations, got shape {s.shape}")
        return "diag", s.copy()
    if s.ndim == 2:
        if s.shape != (dims, dims):
            raise ValueError(f"a 2-D sigma is a [{dims}, {dims}] covariance, got shape {s.shape}")
        return "tril", np.ascontiguousarray(np.linalg.cholesky(s))  # (raises LinAlgError unless positive definite)
    raise ValueError(f"sigma must be a scalar, a 1-D or a 2-D array, got {s.ndim} axes")


def inverse_mass_diagonal(imm, dims: int):
    """None (identity), a scalar or a 1-D [d] array -> None or the diagonal of M^-1; a dense matrix is not implemented."""
    if imm is None:
        return None
    a = np.asarray(imm.detach().cpu() if isinstance(imm, torch.Tensor) else imm, dtype=np.float64)
    if a.ndim == 2:
        raise NotImplementedError("a dense inverse_mass_matrix is not implemented by the HIP HMC kernels; supported: None (identity), "
                                  "a scalar or a 1-D array of the diagonal")
    if a.ndim == 0:
        a = np.full(dims, float(a))
    if a.shape != (dims,) or not np.all(np.isfinite(a) & (a > 0)):
        raise ValueError(f"inverse_mass_matrix must hold {dims} positive numbers, got shape {a.shape}")
    return a.copy()


def data_transform_forward(T, x: torch.Tensor):
    """(x', log|det dx'/dx|) of a flow's data transform in differentiable torch arithmetic: the bounded stage (logit or probit of the
    unit interval, clipped to [eps, 1 - eps]) and the affine stage of `CompositeTransform.forward`.  The HIP transform kernels carry no
    gradient; periodic parameters have no smooth forward map."""
    if T._periodic.any():
        raise NotImplementedError("HMC needs the gradient of the proposal density: a flow with periodic parameters is not supported")
    kind = torch.as_tensor(T._kind, device=x.device)
    v, logj = x, torch.zeros(x.shape[0], dtype=x.dtype, device=x.device)
    if T._kind.any():
        b = kind != 0
        lo = torch.as_tensor(np.where(T._kind != 0, T._lower, 0.0), dtype=x.dtype, device=x.device)
        up = torch.as_tensor(np.where(T._kind != 0, T._upper, 1.0), dtype=x.dtype, device=x.device)
        u = ((x - lo) / (up - lo)).clamp(T.eps, 1.0 - T.eps)
        if (T._kind == 1).any():
            w = torch.log(u) - torch.log1p(-u)
            lj = -torch.log(u) - torch.log1p(-u)
        else:
            w = torch.erfinv(2.0 * u - 1.0) * math.sqrt(2.0)
            lj = 0.5 * (math.log(2.0 * math.pi) + w * w)
        v = torch.where(b, w, x)
        logj = logj + torch.where(b, lj, torch.zeros_like(lj)).sum(-1) + T._unit_logj
    if T.affine_transform:
        mean = torch.as_tensor(T._mean, dtype=x.dtype, device=x.device)
        std = torch.as_tensor(T._std, dtype=x.dtype, device=x.device)
        v = (v - mean) / std
        logj = logj + T._affine_logj
    return v, logj


class HipBlackJAXSMC(SMCSampler):
    """The `"blackjax_smc"` sampler (smc/blackjax.py:13-349) with the random-walk and HMC HIP kernels."""

    rng = None
    key = None
    record_dH = False  # diagnostic: keep the energy differences of a mutation's last transition in `last_dH` (a device tensor)
    last_dH = None
    last_nuts = None  # NUTS, global: leapfrog steps per transition, divergent and moved shares of the last mutation; mean depth of its last transition

    @track_calls
    def sample(self, n_samples: int, n_steps: int = None, adaptive: bool = True, target_efficiency: float = 0.5,
               target_efficiency_rate: float = 1.0, n_final_samples: int | None = None, sampler_kwargs: dict | None = None,
               rng_key=None, checkpoint_callback=None, checkpoint_every: int | None = None, checkpoint_file_path: str | None = None,
               resume_from: str | bytes | dict | None = None, rng=None, min_beta_step: float | None = None,
               max_beta_step: float | None = None, max_n_steps: int | None = None,
               beta_tolerance: float = DEFAULT_BETA_TOLERANCE, store_sample_history: bool = True,
               resample_mode: str | None = None, resample_method: str | None = None):
        global _default_logged
        self.sampler_kwargs = dict(sampler_kwargs or {})
        unknown = sorted(set(self.sampler_kwargs) - set(SAMPLER_KWARGS))
        if unknown:
            raise TypeError(f"sampler_kwargs {unknown} are not supported by the blackjax_smc sampler; supported: "
                            f"{', '.join(SAMPLER_KWARGS)}")
        if "algorithm" not in self.sampler_kwargs and not _default_logged:
            logger.info('blackjax_smc: the default algorithm is "hmc" (the reference defaults to "nuts", which is available here on '
                        'request: sampler_kwargs={"algorithm": "nuts"})')
            _default_logged = True
        self.sampler_kwargs.setdefault("n_steps", 5 * self.dims)  # blackjax.py:118
        self.sampler_kwargs.setdefault("algorithm", "hmc")  # (blackjax.py:119: "nuts")
        self.sampler_kwargs.setdefault("step_size", 1e-3)  # blackjax.py:120
        self.sampler_kwargs.setdefault("num_integration_steps", 10)  # blackjax.py:284-286
        self.sampler_kwargs.setdefault("inverse_mass_matrix", None)  # blackjax.py:121
        self.sampler_kwargs.setdefault("sigma", 0.1)  # blackjax.py:122
        self.sampler_kwargs.setdefault("max_num_doublings", 10)  # blackjax.nuts
        self.sampler_kwargs.setdefault("divergence_threshold", 1000.0)  # blackjax.nuts
        if rng_key is None:
            self.key = 42  # blackjax.py:125-128
        elif isinstance(rng_key, (int, np.integer)) and not isinstance(rng_key, bool):
            self.key = int(rng_key)
        else:
            raise TypeError(f"rng_key must be None or an int (the seed of the per-mutation Philox keys); a JAX key cannot be honoured "
                            f"without jax, got {type(rng_key).__name__}")
        self._check_options()
        self.rng = rng or self.rng or np.random.default_rng()
        return super().sample(
            n_samples, n_steps=n_steps, adaptive=adaptive, target_efficiency=target_efficiency,
            target_efficiency_rate=target_efficiency_rate, n_final_samples=n_final_samples, min_beta_step=min_beta_step,
            max_beta_step=max_beta_step, max_n_steps=max_n_steps, checkpoint_callback=checkpoint_callback,
            checkpoint_every=checkpoint_every, checkpoint_file_path=checkpoint_file_path, resume_from=resume_from,
            beta_tolerance=beta_tolerance, store_sample_history=store_sample_history, resample_mode=resample_mode,
            resample_method=resample_method)

    # ---- options ------------------------------------------------------------------------------------------------------------
    def _builtin_densities(self) -> bool:
        """Both target densities and the proposal density are diagonal Gaussian mixtures in x itself."""
        return (isinstance(self._log_likelihood, DiagGaussianMixture) and isinstance(self._log_prior, DiagGaussianMixture)
                and hasattr(self.prior_flow, "device_mixture") and not getattr(self.prior_flow, "_has_transform", lambda: False)())

    def _check_options(self):
        kw = self.sampler_kwargs
        algorithm = str(kw["algorithm"]).lower()
        if algorithm == "nuts" and not hasattr(self.engine, "nuts_mix"):
            raise NotImplementedError('algorithm="nuts" is not implemented by this engine; use "hmc" or "rwmh"')
        if algorithm in RW_ALGORITHMS:
            self._sigma = proposal_scale(kw["sigma"], self.dims)
            return
        if algorithm not in ("hmc", "nuts"):
            raise ValueError(f"Unsupported algorithm: {algorithm}")  # blackjax.py:321
        self._minv = inverse_mass_diagonal(kw["inverse_mass_matrix"], self.dims)
        if int(kw["num_integration_steps"]) < 1 or not float(kw["step_size"]) > 0.0:
            raise ValueError("num_integration_steps must be >= 1 and step_size positive")
        if algorithm == "nuts":
            k = kw["max_num_doublings"]
            if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= NUTS_MAX_DOUBLINGS:
                raise ValueError(f"max_num_doublings must be an integer in 1 .. {NUTS_MAX_DOUBLINGS}, got {k!r}")
            if not float(kw["divergence_threshold"]) > 0.0:  # (a NaN is refused too)
                raise ValueError(f"divergence_threshold must be positive, got {kw['divergence_threshold']!r}")
        if self._transformed():
            raise NotImplementedError(f"algorithm=\"{algorithm}\" needs identity preconditioning: the HIP transform kernels carry no "
                                      "gradient (use preconditioning=None, or algorithm=\"rwmh\")")
        if self._builtin_densities():
            return
        numpy_callables = [name for name, f in (("log_likelihood", self._log_likelihood), ("log_prior", self._log_prior))
                           if not isinstance(f, (DiagGaussianMixture, GaussianMixture))]
        if numpy_callables and not is_torch_namespace(self.xp):
            raise TypeError(f"algorithm=\"{algorithm}\" takes gradients by torch.autograd: {' and '.join(numpy_callables)} must be "
                            "torch-differentiable callables (construct the sampler with xp=torch), or use algorithm=\"rwmh\"")
        if not (isinstance(self.prior_flow, GaussianFlow) or hasattr(self.prior_flow, "_to_latent")):
            raise TypeError(f"algorithm=\"{algorithm}\" needs a proposal flow with differentiable torch modules, got "
                            f"{type(self.prior_flow).__name__}")

    # ---- the mutation -------------------------------------------------------------------------------------------------------
    def mutate(self, particles, beta, n_steps=None):
        """smc/blackjax.py:145-349: `n_steps` transitions of every particle's own chain.  The host enqueues the launches and reads
        the accept counts once per chunk of 2048 steps."""
        e, kw = self.engine, self.sampler_kwargs
        nsteps = int(n_steps if n_steps is not None else kw["n_steps"])
        x = particles.x if particles.x.is_contiguous() else particles.x.contiguous()
        ll, lp, lq = particles.log_likelihood, particles.log_prior, particles.log_q
        # one key per mutation: (seed, number of mutations so far); the history travels in checkpoints, so a resumed run goes on
        seed = mutation_seed(self.key if self.key is not None else 42, len(self.history.mcmc_acceptance))
        gid0 = self._gid0(particles)
        algorithm = str(kw["algorithm"]).lower()
        n_global = self._n_global(particles)
        if algorithm == "nuts":
            self.fit_preconditioning_transform(x)
            x_new, stats, depth_sum = self._mutate_nuts(x, ll, lp, lq, beta, nsteps, seed, gid0)
            moved, steps, divergent, acc, depth_sum = self._global_counts([int(v) for v in stats] + [depth_sum])
            # NUTSInfo has no is_accepted: the reference records NaN here (blackjax.py:271-277).  Recorded instead: the mean
            # acceptance statistic of the trees, from integer sums, so equal for every sharding and launch order
            rows = n_global * nsteps
            self.history.mcmc_acceptance.append(float(acc / (4294967296.0 * rows)) if nsteps else float("nan"))
            self.last_nuts = {"mean_depth": float(depth_sum / n_global) if nsteps else float("nan"),  # (of the last transition)
                              "steps_per_transition": float(steps / rows) if nsteps else float("nan"),
                              "divergent_share": float(divergent / rows) if nsteps else float("nan"),
                              "moved_share": float(moved / rows) if nsteps else float("nan")}
        else:
            if algorithm in RW_ALGORITHMS:
                x_new, accepted = self._mutate_rw(x, ll, lp, lq, beta, nsteps, seed, gid0)
            else:
                self.fit_preconditioning_transform(x)
                x_new, accepted = self._mutate_hmc(x, ll, lp, lq, beta, nsteps, seed, gid0)
            accepted = self._global_counts([accepted])[0]
            # blackjax.py:226-227: the mean over particles of the mean over steps = accepts / (particles x steps), over the whole
            # population
            self.history.mcmc_acceptance.append(float(accepted / (n_global * nsteps)) if nsteps else float("nan"))
        if self._global_counts([e.count_nonfinite(lq)[0]])[0]:
            raise ValueError("Log proposal contains NaN values")  # blackjax.py:346-347
        return self._wrap(x_new, ll, lp, lq, beta, like=particles)

    def _mutate_rw(self, x, ll, lp, lq, beta, nsteps, seed, gid0):
        """Random-walk Metropolis-Hastings in the preconditioned space z = T(x): propose / densities / accept per step.  One
        evaluation of the three densities per particle and transition."""
        e = self.engine
        z, logj, T = self._enter_preconditioned(x)
        mode, value = self._sigma
        sigma = value if mode == "scalar" else e.asarray(value)
        self.last_mutation_path = "rwmh split: propose / densities / accept per step (asmc_rw_propose, asmc_mh_accept)"
        accepted = 0
        for t0 in range(0, nsteps, MAX_CHUNK):
            chunk = min(MAX_CHUNK, nsteps - t0)
            for t in range(t0, t0 + chunk):
                y = e.rw_propose(z, sigma, seed, gid0, t, t - t0)
                _, ll_new, lp_new, lq_new, logj_new = self._proposal_densities(y, T, x.dtype)
                e.mh_accept(z, y, beta, ll, lp, lq, ll_new, lp_new, lq_new, seed, gid0, t, t - t0, logj=logj, logj_new=logj_new)
            accepted += int(e.mh_counts(chunk).sum())
        x_new = z if T is None else e.asarray(T.inverse(z)[0], dtype=x.dtype)
        return x_new, accepted

    def _fused_ok(self, x) -> bool:
        e = self.engine
        if not (hasattr(e, "hmc_mix") and self._builtin_densities() and x.dtype == torch.float64 and x.shape[1] <= FUSED_MAX_DIMS):
            return False
        mixes = (self._log_likelihood.device_mixture(e), self._log_prior.device_mixture(e), self.prior_flow.device_mixture(e))
        return all(m.logw.shape[0] <= FUSED_MAX_COMPONENTS for m in mixes)

    def _mutate_hmc(self, x, ll, lp, lq, beta, nsteps, seed, gid0):
        e, kw = self.engine, self.sampler_kwargs
        n, d = x.shape
        eps, n_leap = float(kw["step_size"]), int(kw["num_integration_steps"])
        minv = None if self._minv is None else e.asarray(self._minv)
        accepted = 0
        if self._fused_ok(x):
            # built-in densities: whole transitions in one kernel; one gradient evaluation per launch plus n_leap per transition
            self.last_mutation_path = "hmc fused: built-in densities, whole transitions in one kernel (asmc_hmc_mix)"
            mixes = (self._log_likelihood.device_mixture(e), self._log_prior.device_mixture(e), self.prior_flow.device_mixture(e))
            for t0 in range(0, nsteps, MAX_CHUNK):
                chunk = min(MAX_CHUNK, nsteps - t0)
                self.last_dH = e.hmc_mix(x, ll, lp, lq, beta, *mixes, minv, eps, n_leap, seed, gid0, t0, chunk, want_dH=self.record_dH)
                accepted += int(e.mh_counts(chunk).sum())
                self.n_likelihood_evaluations += n * (1 + n_leap * chunk)
            return x, accepted
        # everything else: gradients by torch.autograd between the leapfrog launches; one gradient evaluation per mutation plus
        # n_leap per transition
        self.last_mutation_path = "hmc split: momentum / leapfrog / accept launches around torch.autograd gradients (asmc_hmc_*)"
        if nsteps == 0:
            return x, 0
        g_cur = self._target_and_grad(x.to(torch.float64), beta)[0]
        for t0 in range(0, nsteps, MAX_CHUNK):
            chunk = min(MAX_CHUNK, nsteps - t0)
            for t in range(t0, t0 + chunk):
                p0 = e.hmc_momentum(n, d, minv, seed, gid0, t, t - t0)
                zt, pt = x.to(torch.float64).clone(), p0.clone()
                e.hmc_leap(zt, pt, g_cur, minv, 0.5 * eps, eps)
                for i in range(n_leap):
                    g_new, ll_new, lp_new, lq_new = self._target_and_grad(zt, beta)
                    last = i == n_leap - 1
                    e.hmc_leap(zt, pt, g_new, minv, 0.5 * eps if last else eps, 0.0 if last else eps)
                flags, self.last_dH = e.hmc_accept(x, zt, p0, pt, minv, beta, ll, lp, lq, ll_new, lp_new, lq_new, seed, gid0, t, t - t0,
                                                   want_dH=self.record_dH)
                g_cur = torch.where(flags[:, None], g_new, g_cur)
            accepted += int(e.mh_counts(chunk).sum())
        return x, accepted

    def _mutate_nuts(self, x, ll, lp, lq, beta, nsteps, seed, gid0):
        """`nsteps` NUTS transitions of every row: (x, the four statistics summed over the transitions, the sum of the last
        transition's depths), this rank's rows."""
        e, kw = self.engine, self.sampler_kwargs
        n, d = x.shape
        eps, maxd, thr = float(kw["step_size"]), int(kw["max_num_doublings"]), float(kw["divergence_threshold"])
        minv = None if self._minv is None else e.asarray(self._minv)
        stats = np.zeros(4, dtype=np.int64)
        info = None
        if self._fused_ok(x):
            # built-in densities: whole transitions in one kernel; one gradient evaluation per launch plus one per leapfrog step
            self.last_mutation_path = "nuts fused: built-in densities, whole transitions in one kernel (asmc_nuts_mix)"
            mixes = (self._log_likelihood.device_mixture(e), self._log_prior.device_mixture(e), self.prior_flow.device_mixture(e))
            for t0 in range(0, nsteps, MAX_CHUNK):
                chunk = min(MAX_CHUNK, nsteps - t0)
                for l0 in range(0, chunk, NUTS_MAX_LAUNCH):
                    k = min(NUTS_MAX_LAUNCH, chunk - l0)
                    info = e.nuts_mix(x, ll, lp, lq, beta, *mixes, minv, eps, maxd, thr, seed, gid0, t0 + l0, k, t0=l0,
                                      want_info=t0 + l0 + k == nsteps)
                    self.n_likelihood_evaluations += n
                st = e.nuts_stats(chunk).sum(axis=0)
                self.n_likelihood_evaluations += int(st[1])
                stats += st
        else:
            # everything else: the population in lockstep, gradients by torch.autograd between the launches; one gradient evaluation
            # per mutation plus one per leaf of the longest tree.  At most max_num_doublings synchronisations per transition
            self.last_mutation_path = "nuts split: select / drift / leaf / merge launches around torch.autograd gradients (asmc_nuts_*)"
            if nsteps:
                z0 = x.to(torch.float64)
                g0, ll0, lp0, lq0 = self._target_and_grad(z0, beta)
                st = e.nuts_state(n, d, maxd, minv, eps, beta, thr)
                e.nuts_set_point(st, z0, g0, ll0, lp0, lq0)
            for t0 in range(0, nsteps, MAX_CHUNK):
                chunk = min(MAX_CHUNK, nsteps - t0)
                for t in range(t0, t0 + chunk):
                    e.nuts_begin(st, seed, gid0, t)
                    for j in range(maxd):
                        e.nuts_select(st)
                        for i in range(1 << j):
                            e.nuts_drift(st)
                            g_new, ll_new, lp_new, lq_new = self._target_and_grad(st.z, beta)
                            e.nuts_leaf(st, i, g_new, ll_new, lp_new, lq_new)
                        if e.nuts_merge(st, j) == 0:
                            break
                    info = e.nuts_finish(st, x, ll, lp, lq, t - t0, want_info=t == nsteps - 1)
                stats += e.nuts_stats(chunk).sum(axis=0)
        depth_sum = int(info[:, 0].sum()) if info is not None else 0
        return x, stats, depth_sum

    # ---- differentiable densities (split HMC, split NUTS) --------------------------------------------------------------------------------
    def _flow_log_prob_torch(self, x: torch.Tensor) -> torch.Tensor:
        """log q(x) through the flow's differentiable torch modules (the path training uses), fp64 outside the flow's layers."""
        f = self.prior_flow
        logj = None
        if getattr(f, "_has_transform", lambda: False)():
            x, logj = data_transform_forward(f.data_transform, x)
        if isinstance(f, GaussianFlow):
            mu = torch.as_tensor(f.mu, dtype=x.dtype, device=x.device)
            sigma = torch.as_tensor(f.sigma, dtype=x.dtype, device=x.device)
            r = (x - mu) / sigma
            lq = -0.5 * (r * r).sum(-1) - torch.log(sigma).sum() - 0.5 * f.dims * math.log(2 * math.pi)
        else:
            z, ladj = f._to_latent(x.to(dtype=f.dtype, device=f.device))
            lq = (f._base_logp(z) + ladj).to(dtype=torch.float64, device=x.device)
        return lq if logj is None else lq + logj

    def _target_and_grad(self, z: torch.Tensor, beta: float):
        """(gradient of the tempered log-target, ll, lp, lq) at the fp64 rows z.  Rows whose log-target is not finite contribute no
        gradient; they are rejections whatever the trajectory does."""
        with torch.enable_grad():
            leaf = z.detach().clone().requires_grad_(True)
            # the callables see a view, never the leaf: `torch.asarray(t)` clears requires_grad of a leaf in place (a callable that
            # does this to the view only detaches its own term: the trajectory stays reversible, the accept step exact)
            zz = leaf.view_as(leaf)
            lq = self._flow_log_prob_torch(zz)
            lp, ll = self._eval_prior_likelihood(zz, lq, differentiable=True)
            lpt = (1.0 - beta) * lq + beta * (ll + lp)
            total = torch.where(torch.isfinite(lpt), lpt, torch.zeros_like(lpt)).sum()
            g = torch.autograd.grad(total, leaf, allow_unused=True)[0] if total.requires_grad else None
        if g is None:
            g = torch.zeros_like(z)
        return g.to(torch.float64).contiguous(), ll.detach(), lp.detach(), lq.detach()
