"""The "emcee_smc" sampler on the CPU test double: the facade, the reference's integration scenario, emcee's checks and options,
the history fields, the split, the stationarity of the move, and a two-rank gloo run.

Specification: reference src/aspire/samplers/smc/emcee.py:14-89 with emcee v3's documented StretchMove / RedBlueMove defaults
(emcee is absent: DESIGN.md §3.12 is this repository's reading).  The device kernels are checked against tests/stretch_ref.py in
tests/test_gpu_emcee_smc.py.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

from stretch_ref import StretchOracleEngine
import stretch_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class StretchMove:
    """Stand-in for emcee.moves.StretchMove (emcee is not installed): the sampler reads the type's name and `.a`."""

    def __init__(self, a=2.0):
        self.a = a


class DEMove:
    pass


def _sampler(d, eng=None, seed=4, **kw):
    from aspire_amd.flows import GaussianFlow
    from aspire_amd.samplers.emcee_smc import HipEmceeSMC
    from aspire_amd.targets import DiagGaussianMixture

    eng = eng or StretchOracleEngine()
    lik = DiagGaussianMixture.isotropic(d, normalized=False)
    return HipEmceeSMC(log_likelihood=lik, log_prior=lik, dims=d, prior_flow=GaussianFlow(d, sigma=2.0, engine=eng, seed=3), xp=np,
                       engine=eng, rng=np.random.default_rng(seed), **kw)


def test_philox_restatement_matches_the_oracle(oracle):
    g = np.random.default_rng(0)
    ctr = g.integers(0, 2**32, size=(300, 4), dtype=np.uint64)
    key = g.integers(0, 2**32, size=(300, 2), dtype=np.uint64)
    for i in range(300):
        ref = oracle.philox4x32_10(ctr[i].astype(np.uint32), key[i].astype(np.uint32))
        mine = S.philox4x32_10(*(ctr[i, c:c + 1] for c in range(4)), int(key[i, 0]), int(key[i, 1]))
        assert [int(v) for v in ref] == [int(w[0]) for w in mine]


def test_sample_posterior_emcee_smc_returns_samples_with_evidence(monkeypatch):
    """Before this sampler, `sample_posterior(sampler="emcee_smc")` raised `ValueError: Unknown sampler type`."""
    from aspire_amd import Aspire, Samples
    from aspire_amd import samples as samples_mod
    from aspire_amd.samplers.emcee_smc import HipEmceeSMC
    from aspire_amd.targets import DiagGaussianMixture

    monkeypatch.setattr(samples_mod, "_default_engine", StretchOracleEngine())  # (no GPU in this suite)
    d = 2
    lik = DiagGaussianMixture.isotropic(d, normalized=False)
    aspire = Aspire(log_likelihood=lik, log_prior=lik, dims=d, flow_backend="gaussian")
    aspire.fit(Samples(1.5 * np.random.default_rng(0).normal(size=(500, d))))
    assert aspire.get_sampler_class("emcee_smc") is HipEmceeSMC
    out = aspire.sample_posterior(n_samples=200, sampler="emcee_smc", sampler_kwargs={"nsteps": 5}, engine=StretchOracleEngine(),
                                  rng=np.random.default_rng(1))
    assert len(out.x) == 200 and np.isfinite(float(out.log_evidence)) and np.isfinite(float(out.log_evidence_error))
    assert isinstance(aspire.sampler, HipEmceeSMC)


@pytest.fixture
def h5(monkeypatch):
    from fake_h5 import FakeFile

    from aspire_amd import io
    from aspire_amd import samples as samples_mod

    monkeypatch.setattr(io, "open_h5", lambda path, mode="r": FakeFile(path, mode))
    monkeypatch.setattr(io, "h5py_available", lambda: True)
    monkeypatch.setattr(samples_mod, "_default_engine", StretchOracleEngine())
    return io


@pytest.mark.parametrize("xp_name", ["numpy", "torch"])
@pytest.mark.parametrize("bounded_to_unbounded", [True, False])
def test_reference_integration_scenario(h5, tmp_path, bounded_to_unbounded, xp_name):
    """Reference tests/integration_tests/test_integration.py:11-48 with conftest.py:151-160's "emcee_smc" config, restated
    as tests/test_reference_integration.py restates it for "smc"."""
    from test_reference_integration import _fixtures

    from aspire_amd import Aspire, Samples

    dims, parameters, prior_bounds, xp, log_likelihood, log_prior, init = _fixtures(xp_name)
    samples = Samples(init if xp is np else torch.as_tensor(init), xp=xp)
    aspire = Aspire(log_likelihood=log_likelihood, log_prior=log_prior, dims=dims, parameters=parameters, prior_bounds=prior_bounds,
                    flow_matching=False, bounded_to_unbounded=bounded_to_unbounded, flow_backend="zuko")
    aspire.fit(samples, n_epochs=5)
    out = aspire.sample_posterior(n_samples=100, sampler="emcee_smc", adaptive=True,
                                  sampler_kwargs={"nsteps": 10, "progress": False}, engine=StretchOracleEngine(),
                                  rng=np.random.default_rng(3))
    assert len(out.x) == 100 and out.parameters == parameters and np.isfinite(float(out.log_evidence))
    x = np.asarray(out.x if xp is np else out.x.cpu())
    assert np.all(np.abs(x) <= 10.0) and abs(x.mean() - 2.0) < 0.6
    with h5.open_h5(tmp_path / "test_integration_emcee_smc.h5", "w") as h5_file:
        aspire.save_config(h5_file)
        samples.save(h5_file, path="posterior_samples")


def test_fewer_walkers_than_twice_the_dimension():
    d = 8
    with pytest.raises(RuntimeError, match="It is unadvisable to use a red-blue move with fewer walkers than twice the number of dimensions."):
        _sampler(d).sample(10, sampler_kwargs={"nsteps": 2}, store_sample_history=False)
    post = _sampler(d).sample(10, sampler_kwargs={"nsteps": 2, "live_dangerously": True}, store_sample_history=False)
    assert len(post.x) == 10 and np.isfinite(float(post.log_evidence))


def test_stretch_move_scale_and_unsupported_moves():
    from aspire_amd.samplers.emcee_smc import stretch_move_settings

    assert stretch_move_settings(None) == (2.0, False)
    assert stretch_move_settings(StretchMove(1.5)) == (1.5, False)
    runs = {}
    for name, moves in (("default", None), ("a2", StretchMove(2.0)), ("a1.5", StretchMove(1.5))):
        sp = _sampler(2)
        post = sp.sample(256, sampler_kwargs={"nsteps": 4, "moves": moves}, store_sample_history=False)
        runs[name] = (np.asarray(post.x), list(sp.history.mcmc_acceptance))
    assert np.array_equal(runs["default"][0], runs["a2"][0])  # StretchMove(2.0) is the default move
    assert not np.array_equal(runs["default"][0], runs["a1.5"][0])
    assert runs["a1.5"][1] != runs["default"][1]
    for bad in (DEMove(), [StretchMove()], "stretch"):
        with pytest.raises(NotImplementedError, match="StretchMove"):
            _sampler(2).sample(64, sampler_kwargs={"nsteps": 2, "moves": bad}, store_sample_history=False)
    with pytest.raises(TypeError, match="thin_by"):
        _sampler(2).sample(64, sampler_kwargs={"nsteps": 2, "thin_by": 2}, store_sample_history=False)


def test_history_lengths_and_ranges():
    d = 3
    sp = _sampler(d)
    post = sp.sample(512, sampler_kwargs={"nsteps": 40, "progress": False}, n_final_samples=600, store_sample_history=False)
    h = sp.history
    assert len(post.x) == 600
    assert len(h.mcmc_acceptance) == len(h.beta) + 1 == len(h.mcmc_autocorr)  # + the final mutation
    assert h.mcmc_step_size == []
    for acc in h.mcmc_acceptance:
        assert 0.05 < acc < 1.0
    for tau in h.mcmc_autocorr:
        assert np.shape(tau) == (d,) and np.all(np.isfinite(tau)) and np.all(tau > 0.5)
    assert sp.sampler_kwargs["nsteps"] == 40 and sp.sampler_kwargs["progress"] is False


@pytest.mark.parametrize("phi", [0.5, 0.8])
def test_integrated_time_of_ar1_chains(phi):
    from aspire_amd.samplers.emcee_smc import integrated_time

    g = np.random.default_rng(7)
    n_t, n_w, d = 4000, 32, 2
    x = np.empty((n_t, n_w, d))
    x[0] = g.normal(size=(n_w, d)) / math.sqrt(1 - phi * phi)
    for t in range(1, n_t):
        x[t] = phi * x[t - 1] + g.normal(size=(n_w, d))
    tau = integrated_time(x, c=5, tol=50, quiet=True)
    assert np.all(np.abs(tau / ((1 + phi) / (1 - phi)) - 1) < 0.1), tau
    with pytest.raises(RuntimeError, match="shorter than 50 times"):
        integrated_time(x[:40], quiet=False)


@pytest.mark.parametrize("n", [2, 3, 7, 8, 4096, 4097])
def test_split_halves_and_bijection(n):
    seed = 0x1234_5678_9ABC
    s = S.sigma(np.arange(n), n, 3, 0, seed)
    assert sorted(s.tolist()) == list(range(n))
    assert np.array_equal(S.sigma_inv(s, n, 3, 0, seed), np.arange(n))
    assert int((s % 2 == 0).sum()) == (n + 1) // 2 and int((s % 2 == 1).sum()) == n // 2
    for h in (0, 1):
        k, j, u, ua = S.draws(n, h, 3, 0, seed)
        assert len(k) == (n + 1 - h) // 2 and np.all(s[k] % 2 == h) and np.all(s[j] % 2 == 1 - h)
        assert np.all((u > 0) & (u < 1)) and np.all((ua > 0) & (ua < 1))
    if n >= 7:
        assert not np.array_equal(s, S.sigma(np.arange(n), n, 4, 0, seed))  # the split changes with the step
        assert not np.array_equal(s, S.sigma(np.arange(n), n, 3, 1, seed))  # ... and with the shard


def _correlated_gaussian_run(log_factor=True, n=4000, steps=100, seed=11):
    cov = np.array([[1.0, 0.9], [0.9, 1.0]])
    prec = np.linalg.inv(cov)
    g = np.random.default_rng(seed)
    x = g.multivariate_normal([0.0, 0.0], cov, size=n)

    def logp(z):
        return -0.5 * np.einsum("ni,ij,nj->n", z, prec, z)

    ll, zero = logp(x), np.zeros(n)
    lp, lq = zero.copy(), zero.copy()
    for t in range(steps):
        for h in (0, 1):
            y, logf, _, _ = S.propose(x, h, 2.0, 99, 0, t, log_factor=log_factor)
            z = np.zeros(len(y))
            S.accept(x, h, y, logf, 1.0, ll, lp, lq, logp(y), z, z, 99, 0, t)
    return x, cov


def test_numpy_move_keeps_a_correlated_gaussian_stationary():
    """At beta = 1 the move leaves N(0, Sigma) invariant; without the (d - 1) log zz factor it does not (checked by hand: the
    ensemble then contracts, its covariance ends far outside the tolerance)."""
    x, cov = _correlated_gaussian_run()
    assert np.all(np.abs(x.mean(axis=0)) < 0.1)
    np.testing.assert_allclose(np.cov(x.T), cov, atol=0.1)


def _gloo_worker(rank, world, port, out_dir):
    import torch.distributed as dist

    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from stretch_ref import StretchOracleEngine as Eng

    from aspire_amd.comm import TorchDistComm
    from aspire_amd.flows import GaussianFlow
    from aspire_amd.samplers.emcee_smc import HipEmceeSMC
    from aspire_amd.targets import DiagGaussianMixture

    d, eng = 4, Eng()
    lik = DiagGaussianMixture.isotropic(d, normalized=False)
    sp = HipEmceeSMC(log_likelihood=lik, log_prior=lik, dims=d, prior_flow=GaussianFlow(d, sigma=2.0, engine=eng, seed=3), xp=np,
                     engine=eng, comm=TorchDistComm(torch.device("cpu")), rng=np.random.default_rng(4 + 100 * rank))
    post = sp.sample(2048, sampler_kwargs={"nsteps": 10}, store_sample_history=False)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), beta=np.array(sp.history.beta), logz=float(post.log_evidence),
             acc=np.array(sp.history.mcmc_acceptance), tau=np.array(sp.history.mcmc_autocorr), n=len(post.x),
             counts=eng.stretch_counts(10), x=np.asarray(post.x))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_run(tmp_path):
    """Each rank's shard is its own ensemble; acceptance is the global fraction; every rank appends rank 0's autocorrelation
    time; log Z against the closed form (d/2) log pi."""
    from test_dist_gloo import spawn_ranks

    spawn_ranks(_gloo_worker, 2, lambda port: (2, port, str(tmp_path)))
    r0, r1 = (np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(2))
    assert int(r0["n"]) + int(r1["n"]) == 2048  # (owner layout: offspring stay on their ancestor's rank, the shards are ragged)
    assert np.array_equal(r0["beta"], r1["beta"]) and float(r0["logz"]) == float(r1["logz"])
    assert np.array_equal(r0["acc"], r1["acc"]) and np.array_equal(r0["tau"], r1["tau"], equal_nan=True)
    # the global fraction of the last mutation, from both ranks' local counts
    local = int(r0["counts"].sum()) + int(r1["counts"].sum())
    assert float(r0["acc"][-1]) == local / (2048 * 10)
    assert not np.array_equal(r0["counts"], r1["counts"])  # two ensembles, two streams
    assert abs(float(r0["logz"]) - 2.0 * math.log(math.pi)) < 0.3
