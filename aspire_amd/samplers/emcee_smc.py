"""The `"emcee_smc"` sampler: the SMC loop of `SMCSampler` with emcee's ensemble stretch move as the mutation.

`HipEmceeSMC` mirrors reference src/aspire/samplers/smc/emcee.py:14-89.  The move is emcee's default, `StretchMove(a=2.0)` on
`RedBlueMove(nsplits=2, randomize_split=True)` (Goodman & Weare 2010), run by this repository's HIP kernels
(csrc/asmc_stretch.hip) instead of the third-party `emcee` package, which is absent: parity with its numpy random stream is
unpinned.  `moves` also takes DEMove, DESnookerMove and weighted lists of moves, one move per step
(`aspire_amd.moves`, csrc/asmc_ensemble.hip).
"""
from __future__ import annotations

import logging

import numpy as np
import torch

from .. import moves as ensemble_moves
from .base import MAX_CHUNK, track_calls
from .smc import DEFAULT_BETA_TOLERANCE, SMCSampler

logger = logging.getLogger(__name__)

# emcee/moves/red_blue.py: the check of RedBlueMove.propose, message included
RED_BLUE_MESSAGE = "It is unadvisable to use a red-blue move with fewer walkers than twice the number of dimensions."
AUTOCORR_WALKERS = 256  # mcmc_autocorr is computed over the z-chains of this many walkers of rank 0
SAMPLER_KWARGS = ("nsteps", "progress", "live_dangerously", "n_final_steps", "flow_sample_on_engine")


def stretch_move_settings(moves) -> tuple[float, bool]:
    """(a, live_dangerously) of `moves`: None (emcee's default StretchMove(a=2.0)) or an object whose type is named
    `StretchMove` - emcee's own class, or a stand-in with the same attributes.  Anything else is not implemented."""
    if moves is None:
        return 2.0, False
    if type(moves).__name__ != "StretchMove":
        raise NotImplementedError(f"moves={moves!r} is not implemented by the HIP stretch kernels; supported: moves=None "
                                  "(emcee's default StretchMove(a=2.0)) or a single StretchMove(a=...)")
    if getattr(moves, "nsplits", 2) != 2 or not getattr(moves, "randomize_split", True):
        raise NotImplementedError("only StretchMove with nsplits=2 and randomize_split=True (emcee's defaults) is implemented")
    a = float(getattr(moves, "a", 2.0))
    if not 1.0 < a < np.inf:
        raise ValueError(f"the stretch scale a must be finite and > 1, got {a}")
    return a, bool(getattr(moves, "live_dangerously", False))


def ensemble_move_settings(engine, moves) -> ensemble_moves.MoveSet:
    """The move set of `moves`.  None or one StretchMove: `stretch_move_settings` as the one spec of the default set - the
    stretch kernels alone, as before the DE and snooker moves existed.  Every other value is parsed by `moves.parse_moves` and
    needs an engine with the DE / snooker entry points, which is checked before any attribute of `moves` is read."""
    if ensemble_moves.is_default_path(moves):
        a, live = stretch_move_settings(moves)
        return ensemble_moves.MoveSet((ensemble_moves.MoveSpec("stretch", 2, a),), (1.0,), live, default=True)
    ensemble_moves.require_engine(engine, moves)
    return ensemble_moves.parse_moves(moves)


def check_walkers(move_set, n: int, d: int, live_dangerously: bool, held: str | None = None) -> None:
    """emcee's check of RedBlueMove.propose, and what the kernels' partner draws need; `held`: how the message counts the n."""
    held = held or f", got {n}"
    if n < 2 * d and not (live_dangerously or move_set.live_dangerously):
        raise RuntimeError(RED_BLUE_MESSAGE)
    if n < 2:
        raise ValueError(f"the stretch move needs at least two walkers{held}")
    if not move_set.default and n < 4:
        raise ValueError(f"the DE and snooker moves need at least four walkers{held}")


def autocorr_length_check(tau: np.ndarray, n_t: int, tol: float, quiet: bool) -> None:
    """emcee's rule on an estimate `tau` from `n_t` steps: tol tau > n_t logs its warning (quiet) or raises."""
    flag = tol * np.asarray(tau) > n_t
    if np.any(flag):
        msg = (f"The chain is shorter than {tol} times the integrated autocorrelation time for {int(np.sum(flag))} parameter(s). "
               f"Use this estimate with caution and run a longer chain!\nN/{tol} = {n_t / tol:.0f};\ntau: {tau}")
        if not quiet:
            raise RuntimeError(msg)
        logger.warning(msg)


def integrated_time(x: np.ndarray, c: float = 5, tol: float = 50, quiet: bool = False) -> np.ndarray:
    """emcee.autocorr.integrated_time of a chain [n_steps, n_walkers, d]: per coordinate, the FFT autocorrelation of every
    walker's chain, averaged over the walkers, taus = 2 cumsum(f) - 1, Sokal's window (the first lag with lag >= c tau).  A chain
    shorter than `tol` tau logs a warning (quiet) or raises.  A coordinate whose chains never move gives NaN, as in emcee."""
    x = np.asarray(x, dtype=np.float64)
    n_t, _, n_d = x.shape
    if n_t == 0:
        return np.full(n_d, np.nan)
    n = 1 << (n_t - 1).bit_length()  # emcee's next_pow_two(n_t)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.fft.fft(x - x.mean(axis=0), n=2 * n, axis=0)
        acf = np.fft.ifft(f * np.conjugate(f), axis=0)[:n_t].real
        acf = acf / acf[0]
        taus = 2.0 * np.cumsum(acf.mean(axis=1), axis=0) - 1.0
        m = np.arange(n_t)[:, None] < c * taus
    windows = np.where(m.any(axis=0), np.argmin(m, axis=0), n_t - 1)
    tau = taus[windows, np.arange(n_d)]
    autocorr_length_check(tau, n_t, tol, quiet)
    return tau


class HipEmceeSMC(SMCSampler):
    """The `"emcee_smc"` sampler (smc/emcee.py:14-89) with the stretch-move HIP kernels."""

    rng = None

    @track_calls
    def sample(self, n_samples: int, n_steps: int = None, adaptive: bool = True, target_efficiency: float = 0.5,
               target_efficiency_rate: float = 1.0, sampler_kwargs: dict | None = None, n_final_samples: int | None = None,
               checkpoint_callback=None, checkpoint_every: int | None = None, checkpoint_file_path: str | None = None,
               resume_from: str | bytes | dict | None = None, rng=None, min_beta_step: float | None = None,
               max_beta_step: float | None = None, max_n_steps: int | None = None,
               beta_tolerance: float = DEFAULT_BETA_TOLERANCE, store_sample_history: bool = True,
               resample_mode: str | None = None, resample_method: str | None = None):
        self.sampler_kwargs = dict(sampler_kwargs or {})
        self.sampler_kwargs.setdefault("nsteps", 5 * self.dims)  # emcee.py:31
        self.sampler_kwargs.setdefault("progress", True)  # emcee.py:32 (accepted; there is no progress bar)
        self.emcee_moves = self.sampler_kwargs.pop("moves", None)  # emcee.py:33
        unknown = sorted(set(self.sampler_kwargs) - set(SAMPLER_KWARGS))
        if unknown:
            raise TypeError(f"sampler_kwargs {unknown} are not supported by the emcee_smc sampler; supported: "
                            f"{', '.join(SAMPLER_KWARGS[:3])} and moves")
        self._move_set = ensemble_move_settings(self.engine, self.emcee_moves)
        self.rng = rng or self.rng or np.random.default_rng()
        return super().sample(
            n_samples, n_steps=n_steps, adaptive=adaptive, target_efficiency=target_efficiency,
            target_efficiency_rate=target_efficiency_rate, n_final_samples=n_final_samples, min_beta_step=min_beta_step,
            max_beta_step=max_beta_step, max_n_steps=max_n_steps, checkpoint_callback=checkpoint_callback,
            checkpoint_every=checkpoint_every, checkpoint_file_path=checkpoint_file_path, resume_from=resume_from,
            beta_tolerance=beta_tolerance, store_sample_history=store_sample_history, resample_mode=resample_mode,
            resample_method=resample_method)

    def mutate(self, particles, beta, n_steps=None):
        """smc/emcee.py:47-89: every rank's shard is its own ensemble of walkers on log_prob(z, beta) (smc/base.py:507-519) in the
        preconditioned space z = T(x); a step's group-sweeps (`moves.run_step`) run on the device, the host enqueues them and
        reads the accept counts once (per 2048 steps)."""
        e, comm, kw, move_set = self.engine, self.comm, self.sampler_kwargs, self._move_set
        nsteps = int(n_steps if n_steps is not None else kw["nsteps"])
        x = particles.x if particles.x.is_contiguous() else particles.x.contiguous()
        n_local, d = x.shape
        check_walkers(move_set, n_local, d, kw.get("live_dangerously", False), f" per rank, this rank holds {n_local}")
        ll, lp, lq = particles.log_likelihood, particles.log_prior, particles.log_q
        z, logj, T = self._enter_preconditioned(x)
        seed = int(self.rng.integers(0, 2**63 - 1, dtype=np.int64))
        shard = int(comm.rank)
        k_chain = min(n_local, AUTOCORR_WALKERS) if comm.rank == 0 else 0
        chain = torch.empty((nsteps, k_chain, d), dtype=z.dtype, device=z.device) if k_chain and nsteps else None
        self.last_mutation_path = move_set.path
        schedule = move_set.schedule(seed, nsteps)  # from the mutation's seed: nothing more is taken from self.rng

        def densities(y):
            return self._proposal_densities(y, T, x.dtype)[1:]

        accepted = 0
        for t0 in range(0, nsteps, MAX_CHUNK):
            chunk = min(MAX_CHUNK, nsteps - t0)
            for t in range(t0, t0 + chunk):
                ensemble_moves.run_step(e, move_set.specs[schedule[t]], d, z, beta, ll, lp, lq, logj, densities, seed, shard, t, t - t0)
                if chain is not None:
                    chain[t].copy_(z[:k_chain])
            accepted += int(e.stretch_counts(chunk).sum())
        n_global = self._n_global(particles)
        accepted = self._global_counts([accepted])[0]
        # emcee's mean(acceptance_fraction) = total accepts / (walkers x steps), over the whole population
        self.history.mcmc_acceptance.append(float(accepted / (n_global * nsteps)) if nsteps else float("nan"))
        tau = np.full(d, np.nan)
        if chain is not None:
            # emcee.py:69-73: discard follows sampler_kwargs["nsteps"], also for the final mutation's n_steps
            tau = integrated_time(chain[int(0.2 * kw["nsteps"]):].cpu().numpy(), c=5, tol=50, quiet=True)
        if comm.sharded:
            tau = np.asarray(comm.all_gather_f64(np.asarray(tau, dtype=np.float64))[0], dtype=np.float64)
        self.history.mcmc_autocorr.append(tau)
        x_new = z if T is None else e.asarray(T.inverse(z)[0], dtype=x.dtype)
        if self._global_counts([e.count_nonfinite(lq)[0]])[0]:
            raise ValueError("Log proposal contains NaN values")
        return self._wrap(x_new, ll, lp, lq, beta, like=particles)
