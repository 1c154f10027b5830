"""The un-fused step loops on the CPU test doubles: for every sampler path that runs user callables between a
propose and an accept launch - how often each callable runs, that the prior runs before the likelihood within a proposal, what the
view handed to them carries, the count of likelihood evaluations and the path the sampler names.

The loops are host-side plumbing shared by all samplers (`MCMCSampler._proposal_densities`, `_pcn_split_steps`,
`_pcn_round_trip_steps`, `moves.run_step`); their arithmetic is checked per sampler elsewhere.  `CASES` is also what a before / after
comparison of two commits runs: the builders use the samplers' public interface only.
"""
import math

import numpy as np
import pytest
import torch

from ensemble_ref import EnsembleOracleEngine
from hmc_ref import HmcOracleEngine
from pt_ref import PTOracleEngine

N, STEPS = 64, 3


class AllOracleEngine(PTOracleEngine, EnsembleOracleEngine, HmcOracleEngine):
    """One double with the entry points of every sampler here."""


class Calls:
    """Counting prior and likelihood of a Gaussian problem: N(1, 1) likelihood (unnormalised), N(0, 4) prior, or the uniform prior
    on [-4, 4]^d of a bounded problem.  Every call is logged as (which, rows, view carries log_q, view carries log_prior)."""

    def __init__(self, d, bounded=False, torch_xp=False):
        self.d, self.bounded, self.torch_xp, self.events = d, bounded, torch_xp, []

    def _log(self, which, s):
        self.events.append((which, len(s.x), getattr(s, "log_q", None) is not None, getattr(s, "log_prior", None) is not None))

    def prior(self, s):
        self._log("prior", s)
        x = np.asarray(s.x, dtype=np.float64)
        if self.bounded:
            return np.where(np.all(np.abs(x) <= 4.0, axis=1), -self.d * math.log(8.0), -np.inf)
        return -0.125 * np.sum(x * x, axis=1) - 0.5 * self.d * math.log(8.0 * math.pi)

    def likelihood(self, s):
        self._log("likelihood", s)
        if self.torch_xp:
            return -0.5 * ((s.x - 1.0) ** 2).sum(-1)
        return -0.5 * np.sum((np.asarray(s.x, dtype=np.float64) - 1.0) ** 2, axis=1)


def _flow(eng, d, sigma=1.5):
    from aspire_amd.flows import GaussianFlow

    return GaussianFlow(d, sigma=sigma, engine=eng, seed=3)


def _box(eng, d, kind="logit"):
    from aspire_amd.transforms import CompositeTransform

    params = [f"x_{i}" for i in range(d)]
    return params, CompositeTransform(parameters=params, prior_bounds={p: (-4.0, 4.0) for p in params}, bounded_to_unbounded=True,
                                      bounded_transform=kind, affine_transform=True, xp=np, engine=eng)


def _common(eng, calls, d, bounded, dtype, sigma=1.5, xp=np, log_prior=None):
    kw = dict(log_likelihood=calls.likelihood, log_prior=log_prior or calls.prior, dims=d, prior_flow=_flow(eng, d, sigma), xp=xp,
              engine=eng, rng=np.random.default_rng(4), dtype=dtype)
    if bounded:
        kw["parameters"], kw["preconditioning_transform"] = _box(eng, d)
    return kw


def smc(eng, d, bounded=False, dtype="float64", **sampler_kwargs):
    from aspire_amd.samplers.smc import HipSMC

    calls = Calls(d, bounded)
    s = HipSMC(**_common(eng, calls, d, bounded, dtype))
    return s, calls, s.sample(N, sampler_kwargs=dict(n_steps=STEPS, **sampler_kwargs), store_sample_history=False)


def emcee_smc(eng, d, bounded=False, moves=None):
    from aspire_amd.samplers.emcee_smc import HipEmceeSMC

    calls = Calls(d, bounded)
    s = HipEmceeSMC(**_common(eng, calls, d, bounded, "float64"))
    kw = dict(nsteps=STEPS) if moves is None else dict(nsteps=STEPS, moves=moves())
    return s, calls, s.sample(N, sampler_kwargs=kw, store_sample_history=False)


def _de_snooker():
    from aspire_amd import DEMove, DESnookerMove

    return [(DEMove(), 0.6), (DESnookerMove(), 0.4)]


def blackjax_rwmh(eng, d):
    from aspire_amd.samplers.blackjax_smc import HipBlackJAXSMC

    calls = Calls(d, True)
    s = HipBlackJAXSMC(**_common(eng, calls, d, True, "float64"))
    return s, calls, s.sample(N, sampler_kwargs=dict(algorithm="rwmh", sigma=0.5, n_steps=STEPS), store_sample_history=False)


def blackjax_hmc(eng, d):
    """Split HMC: a torch likelihood under autograd, the prior a full-covariance `GaussianMixture`."""
    from aspire_amd.samplers.blackjax_smc import HipBlackJAXSMC
    from aspire_amd.targets import GaussianMixture

    calls = Calls(d, torch_xp=True)
    prior = GaussianMixture(np.zeros((1, d)), 4.0 * np.eye(d)[None])
    s = HipBlackJAXSMC(**_common(eng, calls, d, False, "float64", xp=torch, log_prior=prior))
    out = s.sample(N, sampler_kwargs=dict(algorithm="hmc", step_size=0.3, num_integration_steps=2, n_steps=STEPS),
                   store_sample_history=False)
    return s, calls, out


def minipcn(eng, d, bounded=False):
    from aspire_amd.samplers.mcmc import HipMiniPCN

    calls = Calls(d, bounded)
    s = HipMiniPCN(**_common(eng, calls, d, bounded, "float64"))
    return s, calls, s.sample(n_walkers=N, n_steps=STEPS)


def emcee(eng, d, bounded=False):
    from aspire_amd.samplers.mcmc import HipEmcee

    calls = Calls(d, bounded)
    s = HipEmcee(**_common(eng, calls, d, bounded, "float64"))
    return s, calls, s.sample(nwalkers=N, nsteps=STEPS)


def pt_minipcn(eng, d):
    from aspire_amd.samplers.mcmc import HipPTMiniPCN

    calls = Calls(d)
    s = HipPTMiniPCN(**_common(eng, calls, d, False, "float64"))
    return s, calls, s.sample(n_walkers=N // 2, n_temps=2, n_steps=STEPS)


CASES = {
    "smc callables d=4 (session)": lambda e: smc(e, 4),
    "smc callables d=5 (row-major)": lambda e: smc(e, 5),
    "smc callables d=4 fp32": lambda e: smc(e, 4, dtype="float32"),
    "smc callables d=5 fp32": lambda e: smc(e, 5, dtype="float32"),
    "smc preconditioned d=4 fuse_transform on": lambda e: smc(e, 4, True),
    "smc preconditioned d=4 fuse_transform off": lambda e: smc(e, 4, True, fuse_transform=False),
    "smc preconditioned d=5 (row-major)": lambda e: smc(e, 5, True),
    "smc preconditioned d=4 fp32 fuse_transform on": lambda e: smc(e, 4, True, dtype="float32"),
    "smc preconditioned d=4 fp32 fuse_transform off": lambda e: smc(e, 4, True, dtype="float32", fuse_transform=False),
    "emcee_smc default move": lambda e: emcee_smc(e, 4),
    "emcee_smc default move under a transform": lambda e: emcee_smc(e, 4, True),
    "emcee_smc DE + snooker": lambda e: emcee_smc(e, 4, moves=_de_snooker),
    "blackjax_smc rwmh under a transform": lambda e: blackjax_rwmh(e, 4),
    "blackjax_smc split hmc, GaussianMixture prior": lambda e: blackjax_hmc(e, 4),
    "minipcn d=4 (session)": lambda e: minipcn(e, 4),
    "minipcn d=5 (row-major)": lambda e: minipcn(e, 5),
    "minipcn under a transform": lambda e: minipcn(e, 4, True),
    "emcee": lambda e: emcee(e, 4),
    "emcee under a transform": lambda e: emcee(e, 4, True),
    "pt_minipcn generic, 2 rungs": lambda e: pt_minipcn(e, 4),
}

SESSION = "callables: whitened-state session (asmc_pcn_ysplit_*)"
SPLIT = "callables: split propose / accept with the step closed on the stream (asmc_pcn_split_*)"
PRECONDITIONED = "preconditioned chain (z = T(x)): split propose / accept around the transform"
STRETCH = "stretch move: propose / densities / accept per half-sweep (asmc_stretch_*)"

# Recorded from a run of the commit before the loops were shared (129326a), on these doubles: (calls of the prior, calls of the
# likelihood, of those the ones whose view carried log_q, n_likelihood_evaluations, last_mutation_path).  They are not taken from the
# code under test.  (Two temperatures; the MCMC samplers' only view with log_q is the initial draw's.)
EXPECTED = {
    "smc callables d=4 (session)": (7, 7, 7, 448, SESSION),
    "smc callables d=5 (row-major)": (10, 10, 10, 640, SPLIT),
    "smc callables d=4 fp32": (7, 7, 7, 448, SESSION),
    "smc callables d=5 fp32": (10, 10, 10, 640, SPLIT),
    "smc preconditioned d=4 fuse_transform on": (7, 7, 7, 448, PRECONDITIONED),
    "smc preconditioned d=4 fuse_transform off": (7, 7, 7, 448, PRECONDITIONED),
    "smc preconditioned d=5 (row-major)": (10, 10, 10, 640, PRECONDITIONED),
    "smc preconditioned d=4 fp32 fuse_transform on": (7, 7, 7, 448, PRECONDITIONED),
    "smc preconditioned d=4 fp32 fuse_transform off": (7, 7, 7, 448, PRECONDITIONED),
    "emcee_smc default move": (13, 13, 13, 448, STRETCH),
    "emcee_smc default move under a transform": (13, 13, 13, 448, STRETCH),
    "emcee_smc DE + snooker": (19, 19, 19, 448, "ensemble moves (0.6 de + 0.4 snooker), one per step: propose / densities / accept per "
                               "group-sweep (asmc_ensemble_*, asmc_stretch_*)"),
    "blackjax_smc rwmh under a transform": (7, 7, 7, 448, "rwmh split: propose / densities / accept per step (asmc_rw_propose, "
                                            "asmc_mh_accept)"),
    "blackjax_smc split hmc, GaussianMixture prior": (0, 15, 15, 960, "hmc split: momentum / leapfrog / accept launches around "
                                                      "torch.autograd gradients (asmc_hmc_*)"),
    "minipcn d=4 (session)": (4, 4, 1, 256, SESSION + ", recorded from the session's state"),
    "minipcn d=5 (row-major)": (4, 4, 1, 256, SPLIT + ", recorded from the rows"),
    "minipcn under a transform": (4, 4, 1, 256, "preconditioned chain (z = T(x)): " + SPLIT + ", recorded from the rows"),
    "emcee": (7, 7, 1, 256, STRETCH + ", recorded from the rows"),
    "emcee under a transform": (7, 7, 1, 256, STRETCH + ", recorded from the rows"),
    "pt_minipcn generic, 2 rungs": (7, 7, 1, 256, "callables: per rung split propose / accept at beta_r (asmc_pcn_split_*), recorded "
                                    "from the rows; exchange by asmc_pt_swap"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_callables_per_proposal(name):
    s, calls, _ = CASES[name](AllOracleEngine())
    ev = calls.events
    lik = [v for v in ev if v[0] == "likelihood"]
    n_prior = len(ev) - len(lik)
    assert (n_prior, len(lik), sum(v[2] for v in lik), s.n_likelihood_evaluations, s.last_mutation_path) == EXPECTED[name]
    assert s.n_likelihood_evaluations == sum(v[1] for v in lik)
    for i, (which, rows, has_lq, has_lp) in enumerate(ev):
        if which == "prior":
            assert not has_lp
            continue
        assert has_lp, "the likelihood's view carries log_prior"
        if n_prior:  # the prior of the same proposal ran just before, on a view with the same log_q
            assert i > 0 and ev[i - 1] == ("prior", rows, has_lq, False)
