"""The "blackjax_smc" sampler on the CPU test double: the facade, the reference's integration scenario under both algorithms, errors
and defaults, the restatement's own checks (gradient, reversibility, noise stream), the history, and a two-rank gloo run.

Specification: reference src/aspire/samplers/smc/blackjax.py:13-349 (blackjax and jax are absent: DESIGN.md §3.13 is this
repository's reading).  The device kernels are checked against tests/hmc_ref.py in tests/test_gpu_blackjax_smc.py.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

import hmc_ref as H
from hmc_ref import HmcOracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sampler(d, eng=None, seed=4, lik=None, xp=np, **kw):
    from aspire_amd.flows import GaussianFlow
    from aspire_amd.samplers.blackjax_smc import HipBlackJAXSMC
    from aspire_amd.targets import DiagGaussianMixture

    eng = eng or HmcOracleEngine()
    lik = lik or DiagGaussianMixture.isotropic(d, normalized=False)
    return HipBlackJAXSMC(log_likelihood=lik, log_prior=lik, dims=d, prior_flow=GaussianFlow(d, sigma=2.0, engine=eng, seed=3), xp=xp,
                          engine=eng, rng=np.random.default_rng(seed), **kw)


def test_sample_posterior_blackjax_smc_returns_samples_with_evidence(monkeypatch):
    """Before this sampler, `sample_posterior(sampler="blackjax_smc")` raised `ValueError: Unknown sampler type`."""
    from aspire_amd import Aspire, Samples
    from aspire_amd import samples as samples_mod
    from aspire_amd.targets import DiagGaussianMixture

    monkeypatch.setattr(samples_mod, "_default_engine", HmcOracleEngine())  # (no GPU in this suite)
    d = 2
    lik = DiagGaussianMixture.isotropic(d, normalized=False)
    aspire = Aspire(log_likelihood=lik, log_prior=lik, dims=d, flow_backend="gaussian")
    aspire.fit(Samples(1.5 * np.random.default_rng(0).normal(size=(500, d))))
    SamplerClass = aspire.get_sampler_class("blackjax_smc")
    from aspire_amd.samplers.blackjax_smc import HipBlackJAXSMC

    assert SamplerClass is HipBlackJAXSMC
    for kw in ({"algorithm": "rwmh", "sigma": 0.5, "n_steps": 5}, {"step_size": 0.3, "n_steps": 3}):
        out = aspire.sample_posterior(n_samples=200, sampler="blackjax_smc", sampler_kwargs=kw, engine=HmcOracleEngine(),
                                      rng=np.random.default_rng(1))
        assert len(out.x) == 200 and np.isfinite(float(out.log_evidence)) and np.isfinite(float(out.log_evidence_error))
        assert isinstance(aspire.sampler, HipBlackJAXSMC)


def test_noise_streams_are_the_pcn_streams(oracle):
    """hmc_ref's normals / accept uniforms against the oracle's per-particle pCN noise (the device functions the kernels reuse)."""
    seed, gid0, step = 0x0123456789ABCDEF, (1 << 32) - 3, 7  # (the ids cross the 32-bit word)
    for d in (1, 2, 7, 33):
        xi = H.normals(seed, gid0, 9, step, d)
        u = H.accept_uniforms(seed, gid0, 9, step)
        for i in range(9):
            ref_xi, ref_u = oracle.pcn_noise(seed, gid0 + i, step, d)
            np.testing.assert_allclose(xi[i], ref_xi, rtol=1e-12, atol=1e-13)
            assert u[i] == ref_u


@pytest.fixture
def h5(monkeypatch):
    from fake_h5 import FakeFile

    from aspire_amd import io
    from aspire_amd import samples as samples_mod

    monkeypatch.setattr(io, "open_h5", lambda path, mode="r": FakeFile(path, mode))
    monkeypatch.setattr(io, "h5py_available", lambda: True)
    monkeypatch.setattr(samples_mod, "_default_engine", HmcOracleEngine())
    return io


def _scenario(h5, tmp_path, bounded_to_unbounded, xp_name, sampler_kwargs):
    from test_reference_integration import _fixtures

    from aspire_amd import Aspire, Samples

    dims, parameters, prior_bounds, xp, log_likelihood, log_prior, init = _fixtures(xp_name)
    samples = Samples(init if xp is np else torch.as_tensor(init), xp=xp)
    aspire = Aspire(log_likelihood=log_likelihood, log_prior=log_prior, dims=dims, parameters=parameters, prior_bounds=prior_bounds,
                    flow_matching=False, bounded_to_unbounded=bounded_to_unbounded, flow_backend="zuko")
    aspire.fit(samples, n_epochs=5)
    out = aspire.sample_posterior(n_samples=100, sampler="blackjax_smc", adaptive=True, sampler_kwargs=sampler_kwargs,
                                  engine=HmcOracleEngine(), rng=np.random.default_rng(3))
    assert len(out.x) == 100 and out.parameters == parameters and np.isfinite(float(out.log_evidence))
    x = np.asarray(out.x if xp is np else out.x.cpu())
    assert np.all(np.abs(x) <= 10.0) and abs(x.mean() - 2.0) < 0.6
    with h5.open_h5(tmp_path / "test_integration_blackjax_smc.h5", "w") as h5_file:
        aspire.save_config(h5_file)
        samples.save(h5_file, path="posterior_samples")
    return aspire


@pytest.mark.parametrize("xp_name", ["numpy", "torch"])
@pytest.mark.parametrize("bounded_to_unbounded", [True, False])
def test_reference_integration_scenario_rwmh(h5, tmp_path, bounded_to_unbounded, xp_name):
    """Reference tests/integration_tests/test_integration.py:11-48 with conftest.py:161-171's "blackjax_smc" config (rwmh,
    sigma = 0.1, n_steps = 10), restated as tests/test_reference_integration.py restates it for "smc"."""
    aspire = _scenario(h5, tmp_path, bounded_to_unbounded, xp_name, {"algorithm": "rwmh", "sigma": 0.1, "n_steps": 10})
    assert "rwmh split" in aspire.sampler.last_mutation_path


@pytest.mark.parametrize("xp_name", ["numpy", "torch"])
@pytest.mark.parametrize("bounded_to_unbounded", [True, False])
def test_reference_integration_scenario_hmc(h5, tmp_path, bounded_to_unbounded, xp_name):
    """The same scenario with algorithm = "hmc", step_size = 0.1, n_steps = 10.  The gradients come from torch.autograd, so the
    torch callables run (through the trained flow's modules and, when bounded, its data transform restated in torch); the numpy
    callables are refused with the TypeError that says so."""
    kw = {"algorithm": "hmc", "step_size": 0.1, "n_steps": 10}
    if xp_name == "numpy":
        with pytest.raises(TypeError, match="torch-differentiable"):
            _scenario(h5, tmp_path, bounded_to_unbounded, xp_name, kw)
        return
    aspire = _scenario(h5, tmp_path, bounded_to_unbounded, xp_name, kw)
    assert "hmc split" in aspire.sampler.last_mutation_path
    assert all(0.0 < a <= 1.0 for a in aspire.sampler.history.mcmc_acceptance)


def test_errors_and_defaults(caplog):
    from aspire_amd.samplers import blackjax_smc as B
    from aspire_amd.transforms import CompositeTransform

    d = 2
    with pytest.raises(NotImplementedError, match='"hmc" or "rwmh"'):
        _sampler(d).sample(64, sampler_kwargs={"algorithm": "nuts"}, store_sample_history=False)
    with pytest.raises(ValueError, match="Unsupported algorithm"):
        _sampler(d).sample(64, sampler_kwargs={"algorithm": "mala"}, store_sample_history=False)
    with pytest.raises(NotImplementedError, match="dense inverse_mass_matrix"):
        _sampler(d).sample(64, sampler_kwargs={"inverse_mass_matrix": np.eye(d)}, store_sample_history=False)
    params = [f"x_{i}" for i in range(d)]
    T = CompositeTransform(parameters=params, prior_bounds={p: [-10.0, 10.0] for p in params}, bounded_to_unbounded=True,
                           affine_transform=False, engine=HmcOracleEngine())
    with pytest.raises(NotImplementedError, match="identity preconditioning"):
        _sampler(d, preconditioning_transform=T).sample(64, sampler_kwargs={"algorithm": "hmc"}, store_sample_history=False)
    with pytest.raises(TypeError, match="torch-differentiable"):
        _sampler(d, lik=lambda s: -0.5 * np.sum(np.asarray(s.x) ** 2, axis=-1)).sample(64, store_sample_history=False)
    with pytest.raises(TypeError, match="thin_by"):
        _sampler(d).sample(64, sampler_kwargs={"thin_by": 2}, store_sample_history=False)
    with pytest.raises(TypeError, match="rng_key"):
        _sampler(d).sample(64, rng_key="a jax key", store_sample_history=False)
    # defaults (blackjax.py:117-122 except the algorithm), the deviation logged once at INFO
    B._default_logged = False
    with caplog.at_level("INFO", logger=B.__name__):
        sp = _sampler(d)
        sp.sample(64, sampler_kwargs={"n_steps": 1}, store_sample_history=False)
        _sampler(d).sample(64, sampler_kwargs={"n_steps": 1}, store_sample_history=False)
    assert sum('default algorithm is "hmc"' in r.getMessage() for r in caplog.records) == 1
    kw = sp.sampler_kwargs
    assert (kw["algorithm"], kw["step_size"], kw["num_integration_steps"], kw["inverse_mass_matrix"], kw["sigma"]) == ("hmc", 1e-3, 10, None, 0.1)
    assert "hmc fused" in sp.last_mutation_path and sp.key == 42
    sp = _sampler(3)
    sp.sample(64, sampler_kwargs={"algorithm": "random_walk"}, max_n_steps=1, store_sample_history=False)
    assert sp.sampler_kwargs["n_steps"] == 15


def test_sigma_forms_and_mass_forms():
    from aspire_amd.samplers.blackjax_smc import inverse_mass_diagonal, proposal_scale

    assert proposal_scale(0.1, 3) == ("scalar", 0.1)
    mode, v = proposal_scale([0.1, 0.2, 0.3], 3)
    assert mode == "diag" and v.tolist() == [0.1, 0.2, 0.3]
    cov = np.array([[1.0, 0.5, 0.0], [0.5, 2.0, 0.3], [0.0, 0.3, 1.5]])
    mode, L = proposal_scale(cov, 3)  # a [d, d] array is a covariance (the number of axes decides, not len(sigma) == dims)
    assert mode == "tril" and np.allclose(L @ L.T, cov) and np.allclose(L, np.tril(L))
    with pytest.raises(ValueError):
        proposal_scale([0.1, 0.2], 3)
    assert inverse_mass_diagonal(None, 3) is None and inverse_mass_diagonal(2.0, 3).tolist() == [2.0] * 3
    # the three proposal forms move the particles as specified: y - x = sigma xi, sig * xi, L xi
    x = np.random.default_rng(0).normal(size=(50, 3))
    xi = H.normals(5, 10, 50, 2, 3)
    np.testing.assert_allclose(H.rw_propose(x, 0.1, 5, 10, 2) - x, 0.1 * xi, atol=1e-15)
    np.testing.assert_allclose(H.rw_propose(x, np.array([0.1, 0.2, 0.3]), 5, 10, 2) - x, np.array([0.1, 0.2, 0.3]) * xi, atol=1e-15)
    np.testing.assert_allclose(H.rw_propose(x, L, 5, 10, 2) - x, xi @ L.T, atol=1e-14)
    runs = {}
    for name, kw in (("scalar", {"sigma": 0.5}), ("diag", {"sigma": [0.5, 0.5]}), ("cov", {"sigma": 0.25 * np.eye(2)}),
                     ("mass", {"algorithm": "hmc", "step_size": 0.3, "inverse_mass_matrix": [1.0, 1.0]}),
                     ("unit", {"algorithm": "hmc", "step_size": 0.3})):
        sp = _sampler(2)
        post = sp.sample(256, sampler_kwargs=dict({"algorithm": "rwmh", "n_steps": 4}, **kw), store_sample_history=False)
        runs[name] = np.asarray(post.x)
    np.testing.assert_allclose(runs["scalar"], runs["diag"], atol=1e-12)  # the same proposal written three ways
    np.testing.assert_allclose(runs["scalar"], runs["cov"], atol=1e-12)
    np.testing.assert_allclose(runs["mass"], runs["unit"], atol=1e-12)


def test_rng_key_reproduces_and_seeds():
    from aspire_amd.samplers.blackjax_smc import mutation_seed

    assert mutation_seed(42, 3) == int(np.random.SeedSequence([42, 3]).generate_state(1, np.uint64)[0])
    out = []
    for key in (None, 42, 43):
        sp = _sampler(3, seed=9)
        post = sp.sample(256, sampler_kwargs={"step_size": 0.3, "n_steps": 3}, rng_key=key, store_sample_history=False)
        out.append((np.asarray(post.x), float(post.log_evidence)))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]  # None is seed 42
    assert not np.array_equal(out[0][0], out[2][0])


def test_restated_gradient_against_finite_differences_and_autograd():
    from aspire_amd.targets import DiagGaussianMixture

    g = np.random.default_rng(1)
    n, d = 40, 5
    x = g.normal(size=(n, d))
    for C in (1, 3, 8):
        w = g.uniform(0.5, 1.5, size=C)
        mu, var = g.normal(size=(C, d)), g.uniform(0.5, 2.0, size=(C, d))
        mix = DiagGaussianMixture(mu, var, weights=w)
        val, grad = H.mix_value_grad((mix.logw, mix.mu, mix.prec), x)
        np.testing.assert_allclose(val, mix(x), rtol=1e-13)
        h = 1e-5
        for j in range(d):
            e = np.zeros(d)
            e[j] = h
            fd = (H.mix_value_grad((mix.logw, mix.mu, mix.prec), x + e)[0] - H.mix_value_grad((mix.logw, mix.mu, mix.prec), x - e)[0]) / (2 * h)
            np.testing.assert_allclose(grad[:, j], fd, rtol=1e-6, atol=1e-8)
        xt = torch.from_numpy(x).requires_grad_(True)
        mix(xt).sum().backward()
        np.testing.assert_allclose(grad, xt.grad.numpy(), rtol=1e-12, atol=1e-13)
        # the long-double run of the same code agrees with the fp64 one to fp64 rounding
        vl, gl = H.mix_value_grad((mix.logw, mix.mu, mix.prec), x.astype(np.longdouble))
        np.testing.assert_allclose(val, vl.astype(np.float64), rtol=1e-13)
        np.testing.assert_allclose(grad, gl.astype(np.float64), rtol=1e-12, atol=1e-14)


def test_leapfrog_is_reversible_and_second_order():
    g = np.random.default_rng(2)
    n, d = 200, 6
    mixes = [H.random_mixture(g, 3, d), H.random_mixture(g, 1, d), H.random_mixture(g, 1, d)]
    x, p = g.normal(size=(n, d)), g.normal(size=(n, d))
    minv = g.uniform(0.5, 2.0, size=d)
    for mass in (None, minv):
        g0 = H.target(mixes, 0.4, x)[3]
        z, p1, _, _, _, g1 = H.trajectory(mixes, 0.4, x, p, g0, 0.05, 10, mass)
        xb, pb, _, _, _, _ = H.trajectory(mixes, 0.4, z, p1, g1, -0.05, 10, mass)
        np.testing.assert_allclose(xb, x, atol=1e-13)
        np.testing.assert_allclose(pb, p, atol=1e-13)

    def err(eps, L):  # the energy error of a trajectory of length 1
        ll0, lp0, lq0, g0 = H.target(mixes, 0.4, x)
        _, p1, ll1, lp1, lq1, _ = H.trajectory(mixes, 0.4, x, p, g0, eps, L, None)
        return np.abs((H.log_p_t(ll1, lp1, lq1, 0.4) - H.kinetic(p1, None)) - (H.log_p_t(ll0, lp0, lq0, 0.4) - H.kinetic(p, None))).mean()

    assert 3.0 < err(0.1, 10) / err(0.05, 20) < 5.0


def test_hmc_accept_rejects_nan_and_plus_inf():
    n, d = 64, 2
    g = np.random.default_rng(3)
    x, z = g.normal(size=(n, d)), g.normal(size=(n, d))
    p0, p1 = g.normal(size=(n, d)), g.normal(size=(n, d))
    ll, lp, lq = (-g.uniform(1, 2, size=n) for _ in range(3))
    lln, lpn, lqn = ll + 5.0, lp.copy(), lq.copy()  # every finite proposal is far better than the start
    lln[::4] = np.nan
    lln[1::4] = np.inf
    p1[2::8] = np.nan  # a divergent trajectory: NaN kinetic energy, NaN dH
    acc, dH = H.hmc_accept(x.copy(), z, p0, p1, None, 0.7, ll.copy(), lp.copy(), lq.copy(), lln, lpn, lqn, 11, 0, 0)
    assert not acc[::4].any() and not acc[1::4].any() and not acc[2::8].any() and np.isnan(dH[2::8]).all()
    assert acc[3::4].all()


def test_history_lengths_and_ranges():
    for kw in ({"algorithm": "rwmh", "sigma": 0.5, "n_steps": 10}, {"step_size": 0.3, "n_steps": 4}):
        sp = _sampler(3)
        post = sp.sample(512, sampler_kwargs=kw, n_final_samples=600, store_sample_history=False)
        h = sp.history
        assert len(post.x) == 600
        assert len(h.mcmc_acceptance) == len(h.beta) + 1  # + the final mutation
        assert h.mcmc_step_size == [] and h.mcmc_autocorr == []
        assert all(0.0 <= a <= 1.0 for a in h.mcmc_acceptance) and 0.05 < np.mean(h.mcmc_acceptance)
    # one likelihood evaluation per particle and transition (rwmh); one per launch plus num_integration_steps per transition (hmc)
    sp = _sampler(2)
    sp.sample(128, sampler_kwargs={"algorithm": "rwmh", "n_steps": 3}, max_n_steps=1, store_sample_history=False)
    assert sp.n_likelihood_evaluations == 128 + 128 * 3
    sp = _sampler(2)
    sp.sample(128, sampler_kwargs={"step_size": 0.1, "n_steps": 3, "num_integration_steps": 4}, max_n_steps=1, store_sample_history=False)
    assert sp.n_likelihood_evaluations == 128 + 128 * (1 + 3 * 4)


def test_split_path_equals_fused_path_on_the_restatement():
    """The same mixtures as built-ins (fused) and as torch callables (split), on the test double: same particles to rounding.  And
    the cap the device test allows itself - rows whose decision sits within the dH tolerance of log u, at most 2 - holds for the
    restatement on that test's inputs."""
    from aspire_amd.targets import DiagGaussianMixture

    d = 7
    g = np.random.default_rng(70)
    mix = DiagGaussianMixture(g.normal(size=(3, d)), g.uniform(0.5, 2.0, size=(3, d)), weights=[0.2, 0.3, 0.5])
    kw = {"step_size": 0.2, "n_steps": 2, "num_integration_steps": 5}
    a = _sampler(d, lik=mix)
    pa = a.sample(512, sampler_kwargs=kw, store_sample_history=False)
    b = _sampler(d, lik=lambda s: mix(s.x), xp=torch)
    pb = b.sample(512, sampler_kwargs=kw, store_sample_history=False)
    assert "fused" in a.last_mutation_path and "split" in b.last_mutation_path
    assert a.history.mcmc_acceptance == b.history.mcmc_acceptance
    np.testing.assert_allclose(np.asarray(pa.x), np.asarray(pb.x.cpu() if torch.is_tensor(pb.x) else pb.x), rtol=1e-9, atol=1e-9)
    mixes, x, beta, eps, L, seed = H.split_fused_case()
    r64, tol, _, _ = H.dh_tolerance(mixes, beta, x, eps, L, None, seed, 0, 0)
    with np.errstate(all="ignore"):
        near = np.abs(r64["dH"] - np.log(H.accept_uniforms(seed, 0, len(x), 0))) < tol
    assert int(near.sum()) <= 2


def _gloo_worker(rank, world, port, out_dir):
    import torch.distributed as dist

    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from hmc_ref import HmcOracleEngine as Eng

    from aspire_amd.comm import TorchDistComm
    from aspire_amd.flows import GaussianFlow
    from aspire_amd.samplers.blackjax_smc import HipBlackJAXSMC
    from aspire_amd.targets import DiagGaussianMixture

    d = 4
    lik = DiagGaussianMixture.isotropic(d, normalized=False)
    res = {}
    for name, kw in (("rw", {"algorithm": "rwmh", "sigma": 0.5, "n_steps": 4}), ("hmc", {"step_size": 0.3, "n_steps": 2})):
        eng = Eng()
        sp = HipBlackJAXSMC(log_likelihood=lik, log_prior=lik, dims=d, prior_flow=GaussianFlow(d, sigma=2.0, engine=eng, seed=3), xp=np,
                            engine=eng, comm=TorchDistComm(torch.device("cpu")), rng=np.random.default_rng(4))
        sp.shard_layout = "slots"  # reproduces the single-rank particle order
        post = sp.sample(1024, sampler_kwargs=kw, store_sample_history=False)
        res[name + "_x"], res[name + "_acc"] = np.asarray(post.x), np.array(sp.history.mcmc_acceptance)
        res[name + "_beta"], res[name + "_logz"] = np.array(sp.history.beta), float(post.log_evidence)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **res)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_run_gives_the_single_rank_particles(tmp_path):
    """The streams are keyed by the global particle id: two ranks (slot layout) draw what one rank draws, so the particles agree
    (to the rounding of the sharded weight reductions, as for the "smc" sampler in tests/test_dist_gloo.py)."""
    from test_dist_gloo import spawn_ranks

    spawn_ranks(_gloo_worker, 2, lambda port: (2, port, str(tmp_path)))
    r0, r1 = (np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(2))
    for name, kw in (("rw", {"algorithm": "rwmh", "sigma": 0.5, "n_steps": 4}), ("hmc", {"step_size": 0.3, "n_steps": 2})):
        sp = _sampler(4)
        post = sp.sample(1024, sampler_kwargs=kw, store_sample_history=False)
        assert np.array_equal(r0[name + "_beta"], r1[name + "_beta"]) and np.array_equal(r0[name + "_acc"], r1[name + "_acc"])
        np.testing.assert_allclose(r0[name + "_beta"], sp.history.beta, rtol=1e-9)
        assert float(r0[name + "_logz"]) == pytest.approx(float(post.log_evidence), abs=5e-9)
        np.testing.assert_allclose(r0[name + "_acc"], sp.history.mcmc_acceptance, atol=1e-12)
        xs = np.concatenate([r0[name + "_x"], r1[name + "_x"]])
        np.testing.assert_allclose(xs, np.asarray(post.x), rtol=1e-9, atol=1e-9)
        assert abs(float(post.log_evidence) - 2.0 * math.log(math.pi)) < 0.3
