"""The "minipcn" and "emcee" samplers on the CPU test double (tests/chain_ref.py): the facade, the reference's arithmetic of burn-in /
thinning / discard / n_samples / last_step_only, the chain checkpoint, what is never evaluated, the errors, and the moments.

Specification: reference src/aspire/samplers/mcmc.py:14-348 and samples.py:599-806; the chains themselves are this repository's
(neither package is installed).  The recorder's kernels are checked in tests/test_gpu_chain_record.py.
"""
import pickle

import numpy as np
import pytest
import torch

from chain_ref import ChainOracleEngine, moment_z_scores

D = 4
POST_MEAN, POST_VAR = 0.8, 0.8  # N(1, 1) likelihood x N(0, 4) prior per coordinate: precision 1.25, mean 1 / 1.25


def targets(d=D):
    from aspire_amd.targets import DiagGaussianMixture

    return (DiagGaussianMixture.isotropic(d, mean=1.0, var=1.0, normalized=False),
            DiagGaussianMixture.isotropic(d, mean=0.0, var=4.0, normalized=True))


def as_callables(pair):
    return tuple((lambda f: (lambda s: f(s)))(f) for f in pair)


def make(kind, d=D, seed=0, callables=False, eng=None, flow=None, **kw):
    from aspire_amd.flows import GaussianFlow
    from aspire_amd.samplers.mcmc import HipEmcee, HipMiniPCN

    eng = eng or ChainOracleEngine()
    ll, lp = as_callables(targets(d)) if callables else targets(d)
    cls = HipEmcee if kind == "emcee" else HipMiniPCN
    return cls(log_likelihood=ll, log_prior=lp, dims=d, prior_flow=flow or GaussianFlow(d, sigma=1.5, engine=eng, seed=100 + seed), xp=np,
               engine=eng, rng=np.random.default_rng(seed), **kw)


@pytest.fixture
def h5(monkeypatch):
    from fake_h5 import FakeFile

    from aspire_amd import io
    from aspire_amd import samples as samples_mod

    monkeypatch.setattr(io, "open_h5", lambda path, mode="r": FakeFile(path, mode))
    monkeypatch.setattr(io, "h5py_available", lambda: True)
    monkeypatch.setattr(samples_mod, "_default_engine", ChainOracleEngine())
    return io


@pytest.mark.parametrize("sampler,kw,shape,thin,burn", [
    ("minipcn", dict(n_walkers=20, n_steps=12), (12, 20), 1, 0),
    ("minipcn", dict(n_walkers=20, n_steps=12, burnin=2, thin=3), (4, 20), 3, 2),
    ("emcee", dict(nwalkers=20, nsteps=12), (12, 20), None, 0),
    ("emcee", dict(nwalkers=20, nsteps=12, discard=5), (7, 20), None, 5),
])
def test_sample_posterior_returns_mcmc_samples(monkeypatch, sampler, kw, shape, thin, burn):
    """Before these samplers, `sample_posterior(sampler="minipcn")` and `"emcee"` raised `ValueError: Unknown sampler type`."""
    from aspire_amd import Aspire, MCMCSamples, Samples
    from aspire_amd import samples as samples_mod
    from aspire_amd.samplers.mcmc import HipEmcee, HipMiniPCN

    monkeypatch.setattr(samples_mod, "_default_engine", ChainOracleEngine())
    lik, pri = targets(2)
    aspire = Aspire(log_likelihood=lik, log_prior=pri, dims=2, flow_backend="gaussian")
    aspire.fit(Samples(1.5 * np.random.default_rng(0).normal(size=(500, 2))))
    assert aspire.get_sampler_class(sampler) is (HipEmcee if sampler == "emcee" else HipMiniPCN)
    out = aspire.sample_posterior(n_samples=None, sampler=sampler, engine=ChainOracleEngine(), rng=np.random.default_rng(1), **kw)
    assert isinstance(out, MCMCSamples) and isinstance(out.x, np.ndarray)
    assert tuple(out.chain_shape) == shape and out.chain.shape == (*shape, 2) and out.thin == thin and out.burn_in == burn
    assert out.n_steps == shape[0] and out.n_chains == shape[1]
    assert np.all(np.isfinite(out.x)) and np.all(np.isfinite(out.log_likelihood)) and np.all(np.isfinite(out.log_prior))
    lik_at = lik(out.x)
    np.testing.assert_allclose(out.log_likelihood, lik_at, rtol=1e-12, atol=1e-12)  # the carried densities belong to the recorded rows


def test_reference_arithmetic_of_n_samples_and_last_step_only():
    """mcmc.py:229-264 / :288-348: n_walkers defaults to n_samples; the returned object is the processed chain's first n_samples
    rows, flattened, metadata kept; last_step_only returns plain Samples of the walkers' last state and records nothing."""
    from aspire_amd import MCMCSamples, Samples

    full = make("minipcn").sample(n_samples=None, n_walkers=10, n_steps=9)
    cut = make("minipcn").sample(n_samples=10, n_steps=9, burnin=1, thin=2)
    assert cut.chain_shape == (10,) and len(cut) == 10 and cut.thin == 2 and cut.burn_in == 1
    assert np.array_equal(cut.x, full.chain[1::2].reshape(-1, D)[:10])  # same seed, same chain: steps 1, 3, 5, 7
    assert np.array_equal(cut.log_prior, np.asarray(full.log_prior).reshape(9, 10)[1::2].reshape(-1)[:10])
    eng = ChainOracleEngine()
    last = make("minipcn", eng=eng).sample(n_samples=10, n_steps=9, last_step_only=True)
    assert type(last) is Samples and not isinstance(last, MCMCSamples) and eng.chain_allocs == 0
    assert np.array_equal(last.x, full.chain[-1]) and np.array_equal(last.log_likelihood, np.asarray(full.log_likelihood)[-10:])
    assert last.log_q is None and last.log_w is None
    em_full = make("emcee").sample(nwalkers=10, nsteps=9, discard=4)
    em = make("emcee").sample(n_samples=10, nsteps=9, discard=4)
    assert em_full.chain_shape == (5, 10) and em_full.burn_in == 4
    assert em.chain_shape == (10,) and em.burn_in == 4 and np.array_equal(em.x, em_full.x[:10])
    kept_all = make("emcee").sample(nwalkers=10, nsteps=9)
    assert np.array_equal(kept_all.chain[4:], em_full.chain)  # get_chain(discard): the same steps, the first ones dropped


@pytest.mark.parametrize("path_kind,expect", [("fused", "asmc_pcn_mutate"), ("ysplit", "asmc_pcn_ysplit"), ("generic", "asmc_pcn_split")])
def test_minipcn_dispatch_paths_agree(path_kind, expect):
    """Mixture densities at d = 4 run inside asmc_pcn_mutate, callables in the whitened-state session, d = 3 (and any transform)
    on the row-major split path; the first two are the same chain (one specification), bit for bit on this double's fp64."""
    d = 3 if path_kind == "generic" else D
    s = make("minipcn", d=d, callables=path_kind != "fused")
    out = s.sample(n_walkers=12, n_steps=6)
    assert expect in s.last_mutation_path and out.chain_shape == (6, 12)
    if path_kind == "ysplit":
        ref = make("minipcn", d=d).sample(n_walkers=12, n_steps=6)
        np.testing.assert_allclose(out.x, ref.x, rtol=0, atol=1e-12)
    moved = np.any(out.chain[1:] != out.chain[:-1], axis=2).mean()
    assert 0.05 < moved < 0.9  # walkers move, and rejections repeat rows


def test_mixtures_take_the_library_loop_at_every_width_and_without_a_chain():
    """As HipSMC: built-in densities run inside asmc_pcn_mutate whatever d, also when nothing is recorded."""
    for d in (3, 5):
        s = make("minipcn", d=d)
        out = s.sample(n_walkers=12, n_steps=6)
        assert "asmc_pcn_mutate" in s.last_mutation_path and out.chain_shape == (6, 12)
        s2 = make("minipcn", d=d)
        last = s2.sample(n_walkers=12, n_steps=6, last_step_only=True)
        assert "asmc_pcn_mutate" in s2.last_mutation_path and np.array_equal(last.x, out.chain[-1])


def test_chain_under_a_bounded_transform(h5):
    """A chain in z = T(x) (logit of a box): the recorded rows are in x space, inside the box; the path is the generic one."""
    from aspire_amd import Aspire, Samples

    lik, pri = as_callables(targets(2))
    bounds = {"x_0": [-10, 10], "x_1": [-10, 10]}
    for sampler, kw in (("minipcn", dict(n_steps=8)), ("emcee", dict(nsteps=8))):
        aspire = Aspire(log_likelihood=lik, log_prior=pri, dims=2, parameters=list(bounds), prior_bounds=bounds, flow_backend="gaussian")
        aspire.fit(Samples(1.0 + np.random.default_rng(0).normal(size=(400, 2))))
        out = aspire.sample_posterior(n_samples=16, sampler=sampler, engine=ChainOracleEngine(), rng=np.random.default_rng(2),
                                      preconditioning_kwargs={"bounded_to_unbounded": True}, **kw)
        assert len(out) == 16 and np.all(np.abs(out.x) < 10.0)
        if sampler == "minipcn":
            assert "preconditioned" in aspire.sampler.last_mutation_path
        np.testing.assert_allclose(out.log_likelihood, targets(2)[0](out.x), rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("sampler", ["minipcn", "emcee"])
def test_chain_checkpoint_hdf5(h5, tmp_path, sampler):
    """The reference's tests/test_samplers/test_mcmc/test_checkpointing.py, restated: `checkpoint/mcmc_chain` through
    MCMCSamples.save with the attributes; minipcn's file holds the FULL chain (before burn-in and thinning)."""
    from aspire_amd import MCMCSamples

    s = make(sampler, callables=True)
    path = tmp_path / f"{sampler}_ckpt.h5"
    if sampler == "minipcn":
        out = s.sample(n_samples=8, n_steps=5, burnin=1, thin=2, checkpoint_file_path=str(path), checkpoint_every=1)
        iteration, full_shape = 5, (5, 8)
    else:
        out = s.sample(n_samples=None, nwalkers=8, nsteps=4, checkpoint_file_path=str(path), checkpoint_every=1)
        iteration, full_shape = 4, (4, 8)
    assert len(out) > 0
    st = s.last_checkpoint_state
    assert st is not None and st["iteration"] == iteration and st["meta"]["stage"] == "mcmc_chain" and "samples" in st
    assert st["sampler"] == type(s).__name__
    with h5.open_h5(path, "r") as fp:
        loaded = MCMCSamples.load(fp, path="checkpoint/mcmc_chain")
        attrs = fp["checkpoint/mcmc_chain"].attrs
        assert attrs["iteration"] == iteration and attrs["stage"] == "mcmc_chain" and attrs["sampler"] == type(s).__name__
        assert tuple(attrs["chain_shape"]) == full_shape
    assert tuple(loaded.chain_shape) == full_shape and loaded.chain.shape == (*full_shape, D)
    if sampler == "minipcn":
        assert len(loaded) > len(out) and loaded.thin == 1 and loaded.burn_in == 0
        assert np.array_equal(loaded.chain[1::2].reshape(-1, D)[:8], out.x)
    else:
        assert len(loaded) == len(out) and tuple(loaded.chain_shape) == tuple(out.chain_shape)


def test_chain_checkpoint_pickle_route_and_negative_every(tmp_path):
    s = make("minipcn")
    path = tmp_path / "chain.pkl"
    s.sample(n_samples=6, n_steps=4, thin=2, checkpoint_file_path=str(path))
    state = pickle.loads(path.read_bytes())
    assert state["samples"].chain_shape == (4, 6) and state["samples"].chain.shape == (4, 6, D) and state["iteration"] == 4
    s2 = make("minipcn")
    s2.sample(n_samples=6, n_steps=4, checkpoint_file_path=str(tmp_path / "none.pkl"), checkpoint_every=0)
    assert s2.last_checkpoint_state is None and not (tmp_path / "none.pkl").exists()
    with pytest.raises(ValueError, match="HDF5 file"):
        make("minipcn").sample(n_samples=6, n_steps=2, checkpoint_file_path=str(tmp_path / "chain.txt"))


class SpyFlow:
    """Counts what the samplers ask of the proposal."""

    def __init__(self, inner):
        self.inner, self.xp, self.log_prob_calls, self.draws = inner, getattr(inner, "xp", None), 0, 0

    def sample_and_log_prob(self, n):
        self.draws += 1
        return self.inner.sample_and_log_prob(n)

    def log_prob(self, x):
        self.log_prob_calls += 1
        return self.inner.log_prob(x)


@pytest.mark.parametrize("sampler,callables", [("minipcn", False), ("minipcn", True), ("emcee", True)])
def test_proposal_density_is_never_evaluated_during_the_chain(sampler, callables):
    from aspire_amd.flows import GaussianFlow

    eng = ChainOracleEngine()
    spy = SpyFlow(GaussianFlow(D, sigma=1.5, engine=eng, seed=5))
    s = make(sampler, eng=eng, flow=spy, callables=callables)
    out = s.sample(n_samples=None, **(dict(nwalkers=10, nsteps=6) if sampler == "emcee" else dict(n_walkers=10, n_steps=6)))
    assert spy.draws >= 1 and spy.log_prob_calls == 0 and out.log_q is None


def test_non_finite_log_q_raises():
    class BadFlow(SpyFlow):
        def sample_and_log_prob(self, n):
            x, lq = self.inner.sample_and_log_prob(n)
            lq = torch.as_tensor(np.asarray(lq.cpu() if hasattr(lq, "cpu") else lq)).clone()
            lq[1] = float("inf")
            return x, lq

    from aspire_amd.flows import GaussianFlow

    for sampler in ("minipcn", "emcee"):
        eng = ChainOracleEngine()
        s = make(sampler, eng=eng, flow=BadFlow(GaussianFlow(D, sigma=1.5, engine=eng, seed=5)))
        with pytest.raises(ValueError, match="Proposal returned non-finite log probabilities"):
            s.sample(n_samples=10)


def test_initial_walkers_are_redrawn_until_finite():
    """mcmc.py:62-108: rows whose prior or likelihood is not finite are dropped and the flow is asked again."""
    from aspire_amd.flows import GaussianFlow

    lik, pri = targets()

    def holed(samples):
        x = np.asarray(samples.x)
        return np.where(x[:, 0] < 0.5, np.nan, lik(samples))

    eng = ChainOracleEngine()
    spy = SpyFlow(GaussianFlow(D, sigma=1.5, engine=eng, seed=5))
    from aspire_amd.samplers.mcmc import HipMiniPCN

    s = HipMiniPCN(log_likelihood=holed, log_prior=lambda smp: pri(smp), dims=D, prior_flow=spy, xp=np, engine=eng, rng=np.random.default_rng(0))
    out = s.sample(n_samples=None, n_walkers=30, n_steps=5)
    assert spy.draws >= 2 and out.chain_shape == (5, 30)
    assert np.all(np.isfinite(out.log_likelihood)) and np.all(out.x[:, 0] >= 0.5)  # the hole never enters a chain


def test_sharded_comm_raises():
    class TwoRanks:
        sharded, world, rank = True, 2, 0

    for sampler in ("minipcn", "emcee"):
        with pytest.raises(NotImplementedError, match="one rank"):
            make(sampler, comm=TwoRanks()).sample(n_samples=10)


@pytest.mark.parametrize("sampler", ["minipcn", "emcee"])
def test_memory_guard_raises_before_any_allocation(sampler):
    eng = ChainOracleEngine()
    eng.free_bytes = 1000
    spy = SpyFlow(__import__("aspire_amd.flows", fromlist=["GaussianFlow"]).GaussianFlow(D, sigma=1.5, engine=eng, seed=5))
    s = make(sampler, eng=eng, flow=spy)
    need = 6 * 10 * (D * 8 + 16)
    with pytest.raises(ValueError, match=rf"{need} bytes.*1000 bytes are free.*last_step_only"):
        s.sample(n_samples=None, **(dict(nwalkers=10, nsteps=6) if sampler == "emcee" else dict(n_walkers=10, n_steps=6)))
    assert eng.chain_allocs == 0 and spy.draws == 0
    if sampler == "minipcn":  # nothing is recorded then: no guard
        assert len(make(sampler, eng=eng).sample(n_samples=10, n_steps=6, last_step_only=True)) == 10


def test_emcee_rules_of_moves_and_walkers():
    class StretchMove:
        def __init__(self, a=2.0):
            self.a = a

    class DEMove:
        pass

    with pytest.raises(RuntimeError, match="red-blue move"):
        make("emcee").sample(nwalkers=2 * D - 1, nsteps=3)
    assert make("emcee").sample(nwalkers=2 * D - 1, nsteps=3, live_dangerously=True).chain_shape == (3, 2 * D - 1)
    with pytest.raises(NotImplementedError, match="moves"):
        make("emcee").sample(nwalkers=10, nsteps=3, moves=DEMove())
    a = make("emcee").sample(nwalkers=10, nsteps=3, moves=StretchMove(a=3.0))
    assert not np.array_equal(a.x, make("emcee").sample(nwalkers=10, nsteps=3).x)
    with pytest.raises(TypeError, match="not supported"):
        make("emcee").sample(nwalkers=10, nsteps=3, tune=True)
    with pytest.raises(NotImplementedError, match="step_fn"):
        make("minipcn").sample(n_samples=10, n_steps=3, step_fn="rwm")


def test_log_prob_maps_nan_and_plus_inf_to_minus_inf():
    lik, pri = targets()
    vals = {0: np.nan, 1: np.inf, 2: -np.inf}

    def holed(samples):
        out = np.array(lik(samples), dtype=np.float64)
        for i, v in vals.items():
            out[i] = v
        return out

    from aspire_amd.flows import GaussianFlow
    from aspire_amd.samplers.mcmc import HipMiniPCN

    eng = ChainOracleEngine()
    s = HipMiniPCN(log_likelihood=holed, log_prior=lambda smp: pri(smp), dims=D, prior_flow=GaussianFlow(D, engine=eng), xp=np, engine=eng)
    z = np.random.default_rng(0).normal(size=(6, D))
    lp = s.log_prob(z)
    assert isinstance(lp, np.ndarray) and np.all(lp[:3] == -np.inf)
    np.testing.assert_allclose(lp[3:], (lik(z) + pri(z))[3:], rtol=1e-12)


@pytest.mark.parametrize("kind", ["minipcn-fused", "minipcn-ysplit", "minipcn-pcn", "emcee"])
def test_chain_moments_against_the_closed_form(kind):
    """d = 4 Gaussian target (N(1, 1) likelihood, N(0, 4) prior: mean 0.8, variance 0.8), 64 walkers, 400 steps, the first half
    discarded.  Mean and variance per coordinate within 5 standard errors computed from the run's own effective sample size
    (tests/chain_ref.py moment_z_scores).  Checked on this restatement over 8 seeds (rng seeds 0 .. 7, flow seeds 100 .. 107) before
    the bound was fixed: the largest |z| of the 64 statistics was 1.84 for minipcn (both paths: one chain) and 2.70 for emcee."""
    sampler = kind.split("-")[0]
    s = make(sampler, callables=kind != "minipcn-fused", seed=3)
    if sampler == "emcee":
        out = s.sample(nwalkers=64, nsteps=400, discard=200)
    else:
        out = s.sample(n_walkers=64, n_steps=400, burnin=200, step_fn="pcn" if kind.endswith("-pcn") else "tpcn")
    assert out.chain_shape == (200, 64)
    z_mean, z_var = moment_z_scores(np.asarray(out.chain), np.full(D, POST_MEAN), np.full(D, POST_VAR))
    print(kind, "z(mean)", np.round(z_mean, 2), "z(variance)", np.round(z_var, 2), "acceptance", s.history.mcmc_acceptance)
    assert np.all(np.abs(z_mean) < 5.0) and np.all(np.abs(z_var) < 5.0)
    assert 0.1 < s.history.mcmc_acceptance[-1] < 0.8
