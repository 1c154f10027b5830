"""The `"minipcn"`, `"emcee"` and `"pt_minipcn"` samplers: plain MCMC from the proposal flow's draws, every step of every walker kept on
the device.

`HipMiniPCN` and `HipEmcee` mirror reference src/aspire/samplers/mcmc.py:203-348 (`Emcee`, `MiniPCN`).  The transitions are this
repository's pCN / tpCN step kernels and stretch-move kernels (csrc/asmc_pcn*.hip, csrc/asmc_stretch.hip) at beta = 1 with a zero
log q array - the target of an MCMC run has no proposal-density term, so the flow's density is never evaluated after the initial
draw - and the chain is written by the recorder of csrc/asmc_chain.hip.  Neither `minipcn` nor `emcee` is installed: the chains
are this repository's specification, parity with the packages' random streams is unpinned.  `HipPTMiniPCN` runs
a ladder of such chains at inverse temperatures beta_r with replica exchange between them; the reference has the
container and the base class of a tempered sampler (samples.py:810-1205, mcmc.py:351-368) and no concrete one.
"""
from __future__ import annotations

import logging
import math
from types import SimpleNamespace

import numpy as np
import torch

from .._xp import is_torch_namespace, to_numpy
from ..history import SMCHistory
from ..samples import MCMCSamples, PTMCMCSamples, Samples
from ..targets import DiagGaussianMixture
from .. import moves as ensemble_moves
from .base import MAX_CHUNK, MCMCSampler, track_calls
from .emcee_smc import check_walkers, ensemble_move_settings
from .smc import HipSMC

logger = logging.getLogger(__name__)


class ChainSampler(MCMCSampler):
    """What the two samplers share: one rank only, the memory guard, the preconditioned start, the containers."""

    last_mutation_path = None
    _last_chain = None  # the whole chain of the last run as a device container: what get_autocorr_time reduces

    def get_autocorr_time(self, discard: int = 0, thin: int = 1, c: float = 5, tol: float = 50, quiet: bool = False):
        """emcee's `EnsembleSampler.get_autocorr_time` over the chain of the last run: the integrated autocorrelation time per
        coordinate ([d]; the tempered sampler: one row per rung) of the steps `get_chain(discard, thin)` keeps, times `thin`,
        reduced on the device where the chain lies.  A chain shorter than `tol` tau raises, or logs a warning
        when `quiet`.  The one deviation from emcee: emcee estimates on its own chain, which lives in the preconditioned space;
        this is the recorded chain, in x.  The sampler keeps the last run's chain alive on the device for this call."""
        from .emcee_smc import autocorr_length_check

        if self._last_chain is None:
            raise RuntimeError(f"{type(self).__name__}.get_autocorr_time needs a recorded chain: call sample() first "
                               "(without last_step_only)")
        full, discard, thin = self._last_chain, int(discard), int(thin)
        tau = full._tau(c, discard, thin)
        autocorr_length_check(tau, len(range(discard + thin - 1, full._rungs()[0].shape[0], thin)), tol, quiet)
        return thin * tau

    def _keep_chain(self, full, autocorr: bool, discard: int = 0):
        """Remember the run's device container; with `autocorr` fill its `autocorrelation_time` (emcee's defaults, quiet) over
        the steps behind `discard`."""
        self._last_chain = full
        if autocorr:
            full.integrated_autocorr_time(quiet=True, discard=discard)
        return full

    def _single_rank(self):
        if self.comm.sharded:
            raise NotImplementedError(f"the {type(self).__name__} sampler runs on one rank: a sharded chain recorder is not "
                                      "implemented (the SMC samplers shard)")

    def _check_chain_memory(self, n_slots: int, n_walkers: int):
        """Before anything is allocated: the chain's rows and its two density arrays against the device's free memory."""
        elem = 4 if self.x_torch_dtype == torch.float32 else 8
        need = int(n_slots) * int(n_walkers) * (self.dims * elem + 16)
        free = int(self.engine.free_memory())
        if need > free:
            raise ValueError(f"the chain of {n_slots} steps x {n_walkers} walkers x {self.dims} dimensions needs {need} bytes of "
                             f"device memory and {free} bytes are free; use last_step_only=True (where the sampler has it), "
                             "fewer steps or fewer walkers")

    def _start(self, n_walkers: int) -> SimpleNamespace:
        """The run's state, by name: the initial walkers from the flow (mcmc.py:49-110) as their image z in the preconditioned
        space (a copy of x itself under the identity, T None), the carried log-Jacobian (or None) and densities."""
        e = self.engine
        init = self.draw_initial_samples(n_walkers)
        x = init.x if init.x.is_contiguous() else init.x.contiguous()
        ll, lp = e.asarray(init.log_likelihood).clone(), e.asarray(init.log_prior).clone()
        z, logj, T = self._enter_preconditioned(x)
        return SimpleNamespace(z=x.clone() if T is None else z, logj=logj, ll=ll, lp=lp, T=T)

    def _record(self, chain, slot, z, ll, lp, T):
        """Slot <- the row-major state: a copy, or T^-1 of it by the transform's own kernels where T has device tables."""
        e = self.engine
        if T is None:
            e.chain_record(chain, slot, x=z, ll=ll, lp=lp)
        elif hasattr(T, "_tables"):
            e.chain_record(chain, slot, x=z, ll=ll, lp=lp, transform=T._tables()[1])
        else:
            e.chain_record(chain, slot, x=e.asarray(T.inverse(z)[0], dtype=z.dtype), ll=ll, lp=lp)

    def _out(self, samples):
        return samples if is_torch_namespace(self.xp) else samples.to_numpy()


class HipMiniPCN(ChainSampler):
    """The `"minipcn"` sampler (mcmc.py:267-348) on the pCN / tpCN step kernels.

    Specification: the reference distribution of the proposal - Gaussian for `pcn`, Student-t by the EM of
    student_t.py for `tpcn` - is fitted once, to the initial walkers in z = T(x); the step size starts at min(2.38 / sqrt(d), 0.99)
    and adapts after every step by `pcn_adapt`; noise and accept streams are the pCN streams of walker i at step t, keyed by one
    seed drawn from `rng`; chain[t] is the state after transition t + 1."""

    _fit_reference = HipSMC._fit_reference
    _fit_reference_gaussian = HipSMC._fit_reference_gaussian
    _upload_reference = HipSMC._upload_reference
    _check_reference_fit = HipSMC._check_reference_fit

    @track_calls
    def sample(self, n_samples: int | None = None, n_walkers: int | None = None, rng=None, target_acceptance_rate=0.234,
               n_steps=100, thin=1, burnin=0, last_step_only=False, step_fn="tpcn", checkpoint_callback=None,
               checkpoint_every: int | None = None, checkpoint_file_path: str | None = None, autocorr: bool = False):
        """`autocorr`: the returned container arrives with `autocorrelation_time` filled, from the steps behind `burnin` (in
        steps of the unthinned chain)."""
        self._single_rank()
        if autocorr and last_step_only:
            raise ValueError("autocorr=True needs the recorded chain: not with last_step_only=True")
        if step_fn not in ("pcn", "tpcn"):
            raise NotImplementedError(f"step_fn={step_fn!r} is not implemented by the HIP step kernels; use step_fn='tpcn' or 'pcn'")
        e = self.engine
        rng = rng or self.rng or np.random.default_rng()
        if not (n_walkers or n_samples):
            raise ValueError("give n_walkers or n_samples: the number of walkers defaults to n_samples")
        n_walkers, n_steps = int(n_walkers or n_samples), int(n_steps)
        if n_steps < 1:
            raise ValueError("n_steps must be at least 1")
        if not last_step_only:
            self._check_chain_memory(n_steps, n_walkers)
        self.history = SMCHistory()
        self.sampler_kwargs = {"step_fn": step_fn}
        self._pcn_state = {"rho": min(2.38 / math.sqrt(self.dims), 0.99), "step": 0, "nu": None}
        run = self._start(n_walkers)
        z, ll, lp, T = run.z, run.ll, run.lp, run.T
        run.ref = self._fit_reference(z, n_walkers, step_fn)
        run.seed = int(rng.integers(0, 2**63 - 1, dtype=np.int64))
        run.n_steps, run.target = n_steps, float(target_acceptance_rate)
        chain = run.chain = None if last_step_only else e.chain_alloc(n_steps, n_walkers, self.dims, z.dtype)
        run.lq, run.zeros = e.full(n_walkers, 0.0), e.full(n_walkers, 0.0)
        builtin = isinstance(self._log_likelihood, DiagGaussianMixture) and isinstance(self._log_prior, DiagGaussianMixture)
        if T is None and builtin:  # (as HipSMC: the fused kernel at every d; also when nothing is recorded)
            acc = self._steps_fused(run)
        else:
            acc = self._steps_split(run, builtin)
        self._check_reference_fit()
        self.history.mcmc_acceptance.append(float(np.mean(acc)) / n_walkers)
        self.history.mcmc_step_size.append(float(self._pcn_state["rho"]))
        self._last_chain = None
        if last_step_only:
            x = z if T is None else e.asarray(T.inverse(z)[0], dtype=z.dtype)
            out = Samples(x=x, xp=torch, parameters=self.parameters)
            out.log_likelihood, out.log_prior = ll, lp  # (set afterwards: no importance weights)
            return self._out(out)
        full = MCMCSamples.from_chain(chain=chain.x, log_likelihood=chain.ll, log_prior=chain.lp, parameters=self.parameters,
                                      xp=torch, dtype=self.dtype, thin=1, burn_in=0, engine=e)
        full = self._out(self._keep_chain(full, autocorr, int(burnin)))
        self.checkpoint_mcmc_chain(samples=full, iteration=n_steps, checkpoint_callback=checkpoint_callback,
                                   checkpoint_every=checkpoint_every, checkpoint_file_path=checkpoint_file_path)
        out = full.post_process(burn_in=burnin, thin=thin)
        if n_samples is not None:
            logger.info(f"Subsampling MCMC samples to {n_samples} samples after burn-in and thinning.")
            out = out[:n_samples]
        return out

    def _steps_fused(self, run):
        """Built-in mixture densities, any d: the whole step loop inside asmc_pcn_mutate, which records into the chain target
        set on the context.  The kernel wants a log q mixture; at beta = 1 its value has no weight (the likelihood's
        stands in)."""
        e, chain = self.engine, run.chain
        self.last_mutation_path = "built-in densities: device-side step loop (asmc_pcn_mutate), recorded by its chain target"
        t_ll, t_lp = self._log_likelihood.device_mixture(e), self._log_prior.device_mixture(e)
        st, acc, done = self._pcn_state, [], 0
        try:
            while done < run.n_steps:
                chunk = min(run.n_steps - done, MAX_CHUNK)
                if chain is not None:
                    e.chain_set(chain, done, 1)
                n_acc, _, st["rho"] = e.pcn_mutate(run.z, run.ll, run.lp, run.lq, 1.0, *run.ref[:3], t_ll, t_lp, t_ll, run.seed, 0,
                                                   st["rho"], chunk, done, run.target, 1, "f64", run.ref[3])
                acc.extend(n_acc.tolist())
                done += chunk
        finally:
            if chain is not None:
                e.chain_clear()
        self.n_likelihood_evaluations += run.n_steps * run.z.shape[0]
        return acc

    def _steps_split(self, run, builtin: bool):
        """Every other case: densities between the propose and accept halves (`_pcn_split_steps`).  Callables under the identity
        at d in {4, 8, 16, 32} run as the whitened-state session, which the recorder reads; every other width, and every chain in
        a preconditioned space, on the row-major state."""
        e, T, chain = self.engine, run.T, run.chain

        def densities(z_prop):
            return self._proposal_densities(z_prop, T, z_prop.dtype, run.zeros)

        def record(t, sess):
            if sess is not None:
                e.chain_record(chain, t, sess=sess, ll=run.ll, lp=run.lp)
            else:
                self._record(chain, t, run.z, run.ll, run.lp, T)

        acc, in_session = self._pcn_split_steps(run.z, run.ll, run.lp, run.lq, run.ref, self._pcn_state, densities, beta=1.0,
                                                seed=run.seed, n_steps=run.n_steps, target=run.target, n_global=run.z.shape[0],
                                                logj=run.logj, session=T is None, on_step=None if chain is None else record)
        if in_session:
            self.last_mutation_path = "callables: whitened-state session (asmc_pcn_ysplit_*), recorded from the session's state"
        else:
            self.last_mutation_path = ("preconditioned chain (z = T(x)): " if T is not None else "") + \
                ("built-in densities by their own kernel: " if builtin else "callables: ") + \
                "split propose / accept with the step closed on the stream (asmc_pcn_split_*), recorded from the rows"
        return acc


EMCEE_KWARGS = ("progress", "moves", "live_dangerously")


class HipEmcee(ChainSampler):
    """The `"emcee"` sampler (mcmc.py:203-264): emcee's default move, StretchMove(a) on RedBlueMove(nsplits=2,
    randomize_split=True), by the stretch kernels on log_prob of the preconditioned space.  One step is two
    half-sweeps; the recorder runs after the second.  `moves` / `live_dangerously`: the rules of `HipEmceeSMC`, DEMove, DESnookerMove
    and weighted lists of moves included (one move per step: `aspire_amd.moves`)."""

    @track_calls
    def sample(self, n_samples: int | None = None, nwalkers: int | None = None, nsteps: int = 500, rng=None, discard=0,
               checkpoint_callback=None, checkpoint_every: int | None = None, checkpoint_file_path: str | None = None,
               autocorr: bool = False, **kwargs):
        """`autocorr`: the returned container arrives with `autocorrelation_time` filled, from the kept steps."""
        self._single_rank()
        unknown = sorted(set(kwargs) - set(EMCEE_KWARGS))
        if unknown:
            raise TypeError(f"keyword arguments {unknown} are not supported by the emcee sampler; supported: {', '.join(EMCEE_KWARGS)}")
        e = self.engine
        move_set = ensemble_move_settings(e, kwargs.get("moves"))
        rng = rng or self.rng or np.random.default_rng()
        if not (nwalkers or n_samples):
            raise ValueError("give nwalkers or n_samples: the number of walkers defaults to n_samples")
        nwalkers, nsteps, discard = int(nwalkers or n_samples), int(nsteps), int(discard)
        if not 0 <= discard < nsteps:
            raise ValueError(f"discard must be in 0 .. nsteps - 1, got {discard} of {nsteps} steps")
        check_walkers(move_set, nwalkers, self.dims, kwargs.get("live_dangerously", False))
        self._check_chain_memory(nsteps - discard, nwalkers)
        self.history = SMCHistory()
        run = self._start(nwalkers)
        z, ll, lp, T = run.z, run.ll, run.lp, run.T
        seed = int(rng.integers(0, 2**63 - 1, dtype=np.int64))
        chain = e.chain_alloc(nsteps - discard, nwalkers, self.dims, z.dtype)  # get_chain(discard): those steps are not kept
        lq, zeros = e.full(nwalkers, 0.0), e.full(nwalkers, 0.0)
        self.last_mutation_path = move_set.path + ", recorded from the rows"
        schedule = move_set.schedule(seed, nsteps)

        def densities(y):
            return self._proposal_densities(y, T, y.dtype, zeros)[1:]

        accepted = 0
        for t0 in range(0, nsteps, MAX_CHUNK):
            chunk = min(MAX_CHUNK, nsteps - t0)
            for t in range(t0, t0 + chunk):
                ensemble_moves.run_step(e, move_set.specs[schedule[t]], self.dims, z, 1.0, ll, lp, lq, run.logj, densities, seed, 0,
                                        t, t - t0)
                if t >= discard:
                    self._record(chain, t - discard, z, ll, lp, T)
            accepted += int(e.stretch_counts(chunk).sum())
        self.history.mcmc_acceptance.append(float(accepted / (nwalkers * nsteps)))
        out = MCMCSamples.from_chain(chain=chain.x, log_likelihood=chain.ll, log_prior=chain.lp, parameters=self.parameters,
                                     xp=torch, dtype=self.dtype, burn_in=discard, engine=e)
        out = self._out(self._keep_chain(out, autocorr))
        self.checkpoint_mcmc_chain(samples=out, iteration=nsteps, checkpoint_callback=checkpoint_callback,
                                   checkpoint_every=checkpoint_every, checkpoint_file_path=checkpoint_file_path)
        if n_samples is not None:
            logger.info(f"Subsampling MCMC samples to {n_samples} samples after burn-in.")
            out = out[:n_samples]
        return out


PT_MAX_RUNGS = 64  # include/asmc.h ASMC_PT_MAX_RUNGS
LADDER_LAG, LADDER_TIME = 10.0, 1.0  # the adaptive ladder's t0 and nu (the sweep behind them)


def default_ladder(n_temps: int, beta_min: float) -> np.ndarray:
    """beta_min^(k / (T - 2)) for k = 0 .. T - 2, then 0: geometric from 1 down to beta_min, and the prior itself, which the
    stepping-stone estimator needs.  One rung is the posterior alone, two are posterior and prior."""
    if n_temps < 1:
        raise ValueError("n_temps must be at least 1")
    if n_temps == 1:
        return np.ones(1)
    if not 0.0 < beta_min < 1.0:
        raise ValueError("beta_min must lie in (0, 1)")
    geo = np.ones(1) if n_temps == 2 else float(beta_min) ** (np.arange(n_temps - 1) / (n_temps - 2))
    return np.concatenate((geo, [0.0]))


class HipPTMiniPCN(ChainSampler):
    """The `"pt_minipcn"` sampler: parallel-tempered pCN / tpCN chains with replica exchange and the evidence on the device.

    Specification (this repository's own).  T rungs of W walkers; rung r targets (1 - beta_r) lq + beta_r (ll + lp)
    with lq the prior's value, i.e. lp + beta_r ll.  The T W initial walkers come from `draw_initial_samples`, rung r takes rows
    r W .. (r + 1) W.  Each rung has its own reference distribution, fitted to its walkers at the start (and every `refit_every`
    steps while t < burnin), and its own step size, from min(2.38 / sqrt(d), 0.99), adapted by `pcn_adapt` with the index
    restarting at every call of the step loop.  Rung r, walker w, step t draws the pCN streams of gid = r W + w at step t.  After
    every `swap_every` steps one `asmc_pt_swap` with round index t / swap_every - 1 (0: never).  chain[r, t] is rung r's state
    after the move of step t and before the exchange that may follow it.  `n_samples` only gives the default number of walkers per
    rung - the result is the whole processed chain, which cannot be sliced -, and `n_temps` / `beta_min` are read only when `betas`
    is not given.

    `rung_launch` changes the launches, not the results.  "per_rung" (the default): every rung's steps are an
    `asmc_pcn_mutate` call of its own, which synchronises.  "batched": one `asmc_pt_steps` call steps all rungs, with the rungs' betas,
    references, step sizes and accept counts in device tables; nothing is read back before the run ends.  Its scope is built-in
    mixture densities under the identity transform at d in {4, 8, 16, 32} with the default noise - anything else raises
    NotImplementedError, there is no fallback.  (The batched steps run on x itself; a per-rung call of 4 or more steps runs on
    the whitened state, which agrees with it to rounding only: the two are bit-identical where every segment has fewer than 4
    steps, e.g. `swap_every` in 1 .. 3.)

    `adapt_ladder=True` (batched only; Vousden, Farr & Mandel 2016): after every odd exchange round k with (k + 1) swap_every <=
    burnin - every pair has then been tried once since the last update - `asmc_pt_ladder_adapt` moves the interior betas towards
    equal swap acceptance, with gain kappa = ladder_lag / (ladder_time (m - 1 + ladder_lag)) at update m.  Afterwards the ladder is
    frozen: `betas` and the returned container carry the final ladder, `ladder_history` [n_updates + 1, T] every ladder, and
    `evidence` is computed from the steps at or after `burnin` alone - earlier steps were drawn on other ladders.  The checkpointed
    full chain contains those earlier steps.  `swap_acceptance_kept` is the pairs' acceptance over the exchange rounds behind
    `burnin` (batched runs, adaptive or not; None otherwise: the per-rung path launches nothing it did not launch before)."""

    _fit_reference = HipSMC._fit_reference
    _fit_reference_gaussian = HipSMC._fit_reference_gaussian
    _upload_reference = HipSMC._upload_reference
    _check_reference_fit = HipSMC._check_reference_fit

    rung_acceptance = rung_step_size = swap_acceptance = swap_acceptance_kept = evidence = betas = ladder_history = None

    def log_likelihood_wrapper(self, z):
        """mcmc.py:354-360: log L at x = T^-1(z), for array input."""
        x, _ = self.preconditioning_transform.inverse(z)
        samples = Samples(x, xp=self.xp, dtype=self.dtype)
        samples.log_prior = self.log_prior(samples)
        samples.log_likelihood = self.log_likelihood(samples)
        return to_numpy(samples.log_likelihood)

    def log_prior_wrapper(self, z):
        """mcmc.py:362-368: log pi at x = T^-1(z) plus log|det dT^-1/dz| (the Jacobian is counted here and only here)."""
        x, logj = self.preconditioning_transform.inverse(z)
        return self.log_prior(Samples(x, xp=self.xp, dtype=self.dtype)) + logj

    @track_calls
    def sample(self, n_samples: int | None = None, n_walkers: int | None = None, n_temps: int = 8, betas=None, beta_min: float = 1e-3,
               n_steps: int = 100, swap_every: int = 1, burnin: int = 0, thin: int = 1, step_fn: str = "tpcn",
               target_acceptance_rate: float = 0.234, refit_every: int | None = None, rng=None, checkpoint_callback=None,
               checkpoint_every: int | None = None, checkpoint_file_path: str | None = None, rung_launch: str = "per_rung",
               adapt_ladder: bool = False, ladder_lag: float = LADDER_LAG, ladder_time: float = LADDER_TIME, noise: str = "f64",
               autocorr: bool = False):
        """`autocorr`: the returned container arrives with `autocorrelation_time` [n_temps, d] filled, from the steps behind
        `burnin` (in steps of the unthinned chain); the cold rung's row is appended to `history.mcmc_autocorr`."""
        self._single_rank()
        if step_fn not in ("pcn", "tpcn"):
            raise NotImplementedError(f"step_fn={step_fn!r} is not implemented by the HIP step kernels; use step_fn='tpcn' or 'pcn'")
        if rung_launch not in ("per_rung", "batched"):
            raise ValueError(f"rung_launch must be 'per_rung' or 'batched', got {rung_launch!r}")
        if noise not in ("f64", "f32"):
            raise ValueError(f"noise must be 'f64' or 'f32', got {noise!r}")
        batched = rung_launch == "batched"
        e = self.engine
        rng = rng or self.rng or np.random.default_rng()
        if not (n_walkers or n_samples):
            raise ValueError("give n_walkers or n_samples: the number of walkers per rung defaults to n_samples")
        if betas is None:
            ladder = default_ladder(int(n_temps), float(beta_min))
        else:
            ladder = np.asarray(to_numpy(betas), dtype=np.float64)
            if ladder.ndim != 1 or ladder.size < 1 or ladder[0] != 1.0 or np.any(np.diff(ladder) >= 0) or ladder[-1] < 0:
                raise ValueError("betas must be a 1D array that starts at 1, decreases strictly and stays in [0, 1]")
        n_t = int(ladder.size)
        if n_t > PT_MAX_RUNGS:
            raise ValueError(f"at most {PT_MAX_RUNGS} rungs, got {n_t}")
        W, n_steps, swap_every = int(n_walkers or n_samples), int(n_steps), int(swap_every)
        if n_steps < 1:
            raise ValueError("n_steps must be at least 1")
        if swap_every < 0 or (refit_every is not None and int(refit_every) < 1):
            raise ValueError("swap_every must be non-negative and refit_every positive")
        burnin = int(burnin)
        if adapt_ladder:
            if not batched:
                raise ValueError("adapt_ladder needs rung_launch='batched': the ladder moves on the device")
            if swap_every < 1:
                raise ValueError("adapt_ladder needs swap_every >= 1: the update reads the exchange's acceptance")
            if n_t < 3:
                raise ValueError("adapt_ladder needs at least 3 rungs: the two ends of the ladder are fixed")
            if ladder[-1] != 0.0:
                raise ValueError("adapt_ladder needs a ladder that ends at 0: the hot end is fixed at infinite temperature")
            if burnin < 2 * swap_every:
                raise ValueError("adapt_ladder needs burnin >= 2 swap_every: the ladder moves during burn-in only, after two rounds")
            if burnin >= n_steps:
                raise ValueError("adapt_ladder needs burnin < n_steps: the evidence comes from the steps behind burnin, on the final ladder")
            if not (float(ladder_lag) > 0.0 and float(ladder_time) > 0.0):
                raise ValueError("ladder_lag and ladder_time must be positive")
        self._check_chain_memory(n_t * n_steps, W)
        if hasattr(e, "ensure_capacity"):
            e.ensure_capacity(n_t * W, self.dims)
        self.history = SMCHistory()
        self.sampler_kwargs = {"step_fn": step_fn}
        run = self._start(n_t * W)
        z, logj, ll, lp, T = run.z, run.logj, run.ll, run.lp, run.T
        builtin = isinstance(self._log_likelihood, DiagGaussianMixture) and isinstance(self._log_prior, DiagGaussianMixture)
        if batched:
            why = ("the densities are callables" if not builtin else "the chain runs in a preconditioned space (a transform)" if T is not None
                   else f"noise={noise!r}" if noise != "f64"
                   else f"d={self.dims} is not one of 4, 8, 16, 32 with 16-byte aligned rows" if not e.pt_steps_supported(z) else None)
            if why:
                raise NotImplementedError(f"rung_launch='batched' steps built-in mixture densities under the identity transform at d in "
                                          f"{{4, 8, 16, 32}} with the default noise: {why}; use rung_launch='per_rung'")
        elif noise != "f64" and not (T is None and builtin):
            raise NotImplementedError("noise='f32' is implemented for built-in densities under the identity transform only")
        rows = [slice(r * W, (r + 1) * W) for r in range(n_t)]
        states = [{"rho": min(2.38 / math.sqrt(self.dims), 0.99), "step": 0, "nu": None} for _ in range(n_t)]
        refs = [None] * n_t

        def refit(r):
            self._pcn_state = states[r]
            mu, L, Linv, nu = self._fit_reference(z[rows[r]], W, step_fn)
            refs[r] = (mu.clone(), L.clone(), Linv.clone(), nu)  # (the fit's outputs are views of buffers the next fit reuses)
            self._check_reference_fit()

        for r in range(n_t):
            refit(r)
        seed = int(rng.integers(0, 2**63 - 1, dtype=np.int64))
        chain = e.chain_alloc(n_t * n_steps, W, self.dims, z.dtype)
        x4, ll3, lp3 = chain.x.view(n_t, n_steps, W, self.dims), chain.ll.view(n_t, n_steps, W), chain.lp.view(n_t, n_steps, W)
        chains = [type(chain)(x4[r], ll3[r], lp3[r]) for r in range(n_t)]
        lq = lp.clone()  # the proposal-density slot carries the prior's value: (1 - beta) lq + beta (ll + lp) = lp + beta ll
        betas_dev = e.asarray(ladder)
        counts = torch.zeros(max(n_t - 1, 1), dtype=torch.int64, device=betas_dev.device)
        stepper = self._segment_fused if T is None and builtin else self._segment_generic
        self._noise = noise
        run.lq, run.rows, run.ladder, run.states, run.refs, run.chains = lq, rows, ladder, states, refs, chains
        run.seed, run.target = seed, float(target_acceptance_rate)
        refit_every = None if refit_every is None else int(refit_every)
        accepted, done, n_rounds = np.zeros(n_t), 0, 0
        kept0, rounds0 = None, 0  # (batched) the exchange counts when the kept steps begin
        if batched:
            if burnin <= 0:
                kept0 = counts.clone()
            # what the per-rung path keeps on the host, as device tables; the ladder's history (row 0: the given ladder)
            rho_dev = e.asarray(np.array([st["rho"] for st in states]))
            accept_dev, snap = torch.zeros(n_t, dtype=torch.int64, device=betas_dev.device), torch.zeros_like(counts)
            n_updates = (burnin // swap_every) // 2 if adapt_ladder else 0
            history = torch.zeros((n_updates + 1, n_t), dtype=torch.float64, device=betas_dev.device)
            history[0].copy_(betas_dev)
            t_ll, t_lp = self._log_likelihood.device_mixture(e), self._log_prior.device_mixture(e)
            pack, updates = None, 0
            self.last_mutation_path = ("built-in densities: all rungs in one device-side step loop (asmc_pt_steps) on device tables of "
                                       "beta_r, reference, step size and counts, recorded by its own launch; exchange by asmc_pt_swap"
                                       + ("; ladder adapted by asmc_pt_ladder_adapt" if adapt_ladder else ""))
        try:
            while done < n_steps:
                if done and refit_every and done % refit_every == 0 and done < burnin:
                    for r in range(n_t):
                        refit(r)
                    pack = None
                if batched and pack is None:
                    pack = e.pt_pack(z, n_t, refs, t_ll, t_lp, t_lp)
                stops = [n_steps, done + MAX_CHUNK]
                if swap_every:
                    stops.append((done // swap_every + 1) * swap_every)
                if refit_every and done < burnin:
                    stops.append((done // refit_every + 1) * refit_every)
                chunk = min(stops) - done
                if batched:  # (the adaptation index restarts with the call, as it does per rung)
                    e.pt_steps(pack, z, ll, lp, lq, betas_dev, rho_dev, accept_dev, seed, chunk, done, float(target_acceptance_rate), True,
                               chain=chain, n_slots=n_steps, slot0=done)
                    self.n_likelihood_evaluations += chunk * z.shape[0]
                else:
                    accepted += stepper(run, done, chunk)
                done += chunk
                if swap_every and n_t > 1 and done % swap_every == 0:
                    k = done // swap_every - 1
                    e.pt_swap(z, ll, lp, betas_dev, seed, k, counts, c0=lq, c1=logj)
                    n_rounds += 1
                    if adapt_ladder and k % 2 == 1 and done <= burnin:
                        e.pt_ladder_adapt(W, counts, snap, betas_dev, history, (k + 1) // 2, float(ladder_lag), float(ladder_time))
                        updates += 1
                if batched and kept0 is None and done >= burnin:
                    kept0, rounds0 = counts.clone(), n_rounds
        finally:
            e.chain_clear()
        if batched:  # the one read of the run's tables
            accepted = to_numpy(accept_dev).astype(np.float64)
            self.rung_step_size = np.asarray(to_numpy(rho_dev), dtype=np.float64).copy()
            self.ladder_history = np.asarray(to_numpy(history), dtype=np.float64)[:updates + 1].copy()
            ladder = self.ladder_history[-1].copy()
        else:
            self.rung_step_size = np.array([st["rho"] for st in states])
            self.ladder_history = ladder[None, :].copy()
        self.betas = ladder
        self.rung_acceptance = accepted / (n_steps * W)
        pair_tries = lambda k0: np.array([len(range(k0 + (r - k0) % 2, n_rounds, 2)) for r in range(n_t - 1)], dtype=np.float64) * W  # noqa: E731
        tries = pair_tries(0)
        got = to_numpy(counts)[:n_t - 1].astype(np.float64)  # the one read of the device counts
        self.swap_acceptance = np.divide(got, tries, out=np.zeros(n_t - 1), where=tries > 0)
        if batched:
            if kept0 is None:
                kept0, rounds0 = counts, n_rounds
            tries = pair_tries(rounds0)
            self.swap_acceptance_kept = np.divide(got - to_numpy(kept0)[:n_t - 1].astype(np.float64), tries, out=np.zeros(n_t - 1),
                                                  where=tries > 0)
        else:
            self.swap_acceptance_kept = None
        self.history.mcmc_acceptance.append(float(self.rung_acceptance[0]))
        self.history.mcmc_step_size.append(float(self.rung_step_size[0]))
        full = PTMCMCSamples.from_chain(chain=x4, betas=ladder, log_likelihood=ll3, log_prior=lp3, parameters=self.parameters, xp=torch,
                                        dtype=self.dtype, thin=1, burn_in=0, engine=e)
        if adapt_ladder:  # only the steps on the final ladder
            kept = full.post_process(burn_in=burnin)
            self.evidence = {"thermodynamic_integration": kept.log_evidence_thermodynamic_integration(burn_in_fraction=None),
                             "stepping_stone": kept.log_evidence_stepping_stone(burn_in_fraction=None)}
        else:
            self.evidence = {"thermodynamic_integration": full.log_evidence_thermodynamic_integration(),
                             "stepping_stone": full.log_evidence_stepping_stone() if ladder[-1] == 0.0 else None}
        self._keep_chain(full, autocorr, int(burnin))
        if autocorr:
            self.history.mcmc_autocorr.append(np.asarray(full.autocorrelation_time[0], dtype=np.float64).copy())
        full = self._out(full)
        self.checkpoint_mcmc_chain(samples=full, iteration=n_steps, checkpoint_callback=checkpoint_callback,
                                   checkpoint_every=checkpoint_every, checkpoint_file_path=checkpoint_file_path)
        return full.post_process(burn_in=int(burnin), thin=int(thin))

    def _segment_fused(self, run, t0: int, chunk: int):
        """Built-in mixture densities under the identity transform: per rung one asmc_pcn_mutate call on its row range with the
        prior's mixture as the log q mixture, recorded by the chain target pointed at the rung's block.  Each call synchronises."""
        e, z, states = self.engine, run.z, run.states
        self.last_mutation_path = ("built-in densities: per rung the device-side step loop (asmc_pcn_mutate) at beta_r, recorded by "
                                   "its chain target; exchange by asmc_pt_swap")
        t_ll, t_lp = self._log_likelihood.device_mixture(e), self._log_prior.device_mixture(e)
        acc = np.zeros(len(run.rows))
        for r, sl in enumerate(run.rows):
            mu, L, Linv, nu = run.refs[r]
            e.chain_set(run.chains[r], t0, 1)
            n_acc, _, states[r]["rho"] = e.pcn_mutate(z[sl], run.ll[sl], run.lp[sl], run.lq[sl], float(run.ladder[r]), mu, L, Linv, t_ll,
                                                      t_lp, t_lp, run.seed, r * z[sl].shape[0], states[r]["rho"], chunk, t0, run.target, 1,
                                                      self._noise, nu)
            acc[r] = float(np.sum(n_acc))
        self.n_likelihood_evaluations += chunk * z.shape[0]
        return acc

    def _segment_generic(self, run, t0: int, chunk: int):
        """Callables, and every chain in a preconditioned space: per rung the row-major split loop (`_pcn_split_steps`) at beta_r
        with lq' := lp', recorded from the rows."""
        T = run.T
        builtin = isinstance(self._log_likelihood, DiagGaussianMixture) and isinstance(self._log_prior, DiagGaussianMixture)
        self.last_mutation_path = ("preconditioned chain (z = T(x)): " if T is not None else "") + \
            ("built-in densities by their own kernel: " if builtin else "callables: ") + \
            "per rung split propose / accept at beta_r (asmc_pcn_split_*), recorded from the rows; exchange by asmc_pt_swap"

        def densities(z_prop):
            return self._proposal_densities(z_prop, T, z_prop.dtype, "prior")

        acc = np.zeros(len(run.rows))
        for r, sl in enumerate(run.rows):
            zr, llr, lpr = run.z[sl], run.ll[sl], run.lp[sl]
            n = zr.shape[0]
            n_acc, _ = self._pcn_split_steps(zr, llr, lpr, run.lq[sl], run.refs[r], run.states[r], densities, beta=float(run.ladder[r]),
                                             seed=run.seed, n_steps=chunk, target=run.target, n_global=n, gid0=r * n, step0=t0,
                                             logj=None if run.logj is None else run.logj[sl], session=False,
                                             on_step=lambda t, _: self._record(run.chains[r], t, zr, llr, lpr, T))
            acc[r] = float(np.sum(n_acc))
        return acc
