"""GaussianMixture end to end on the device, against closed forms.

16 seeds per family; z = (log Z - truth) / log_evidence_error must look standard normal by the criterion of
tests/test_gpu_logz_validation.py: |mean z| < 0.6 and 0.55 <= rms z <= 1.5.  Runs are bit-reproducible for a fixed seed.

  (a) correlated Gaussian, d = 8: normalised likelihood N(m, Sigma), condition number 100, standard-normal DiagGaussianMixture
      prior, Gaussian proposal; sampler "smc" with pcn and tpcn.  log Z = log N(m; 0, Sigma + I).
  (b) the reference's basic example at d = 4: DiagGaussianMixture likelihood N(2, 1) under GaussianMixture.uniform(-10, 10);
      log Z = -4 log 20 (the mass outside the box is below 1e-15).
  (c) "blackjax_smc" with algorithm "hmc" on (a): the gradient instantiation of the kernel runs, GaussianMixture.__call__ never.
  (d) one "emcee_smc" run and one "minipcn" chain on (a): path, kernel, finite output; the chain's mean within 5 standard errors.

Configuration.  Case (a) with pcn gives the same sixteen z through the engine's CPU test double and __call__; (a) tpcn, (b) and (c)
have no CPU rehearsal at this population.  (c) needs sixteen transitions of ten leapfrog steps per temperature: six of eight mix too
little (mean z = -1.00).  The criterion is the project's, unchanged.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, SEEDS, D = 1 << 15, 16, 8


def problem_a(d=D):
    """(likelihood, prior, m, Sigma, log Z): eigenvalues of Sigma spread geometrically over [0.1, 10], random eigenvectors."""
    from scipy.stats import multivariate_normal as mvn

    from aspire_amd import DiagGaussianMixture, GaussianMixture

    g = np.random.default_rng(2024)
    Q = np.linalg.qr(g.normal(size=(d, d)))[0]
    Sigma = (Q * np.geomspace(0.1, 10.0, d)) @ Q.T
    Sigma = 0.5 * (Sigma + Sigma.T)
    m = 0.5 * g.normal(size=d)
    truth = float(mvn(np.zeros(d), Sigma + np.eye(d)).logpdf(m))
    return GaussianMixture(m, Sigma), DiagGaussianMixture.isotropic(d), m, Sigma, truth


def posterior_a():
    _, _, m, Sigma, _ = problem_a()
    P = np.linalg.inv(Sigma)
    cov = np.linalg.inv(P + np.eye(D))
    return cov @ (P @ m), cov


def flow_for(eng, d, seed):
    from aspire_amd.flows import GaussianFlow

    return GaussianFlow(d, sigma=1.5, seed=seed, engine=eng)


def z_scores(eng, cls, lik, prior, d, truth, n=N, seeds=SEEDS, **kw):
    z, paths = [], set()
    for s in range(seeds):
        sp = cls(log_likelihood=lik, log_prior=prior, dims=d, prior_flow=flow_for(eng, d, s), xp=np, engine=eng,
                 rng=np.random.default_rng(100 + s))
        out = sp.sample(n, sampler_kwargs=dict(kw), store_sample_history=False)
        z.append((float(out.log_evidence) - truth) / float(out.log_evidence_error))
        paths.add(sp.last_mutation_path)
    return np.array(z), paths


def check(z, what):
    mean, rms = float(z.mean()), float(np.sqrt((z**2).mean()))
    print(f"{what}: z = {np.round(z, 2).tolist()} mean {mean:+.2f} rms {rms:.2f}")
    assert abs(mean) < 0.6 and 0.55 <= rms <= 1.5, f"{what}: mean {mean:+.2f} rms {rms:.2f}"


def census(eng, fn):
    eng.profile(True)
    eng.profile_variants()
    out = fn()
    v = eng.profile_variants()
    eng.profile(False)
    return out, v


def ran(v, frag):
    return sum(c for k, c in v.items() if frag in k)


@pytest.mark.parametrize("step_fn", ["pcn", "tpcn"])
def test_a_correlated_gaussian_smc(hip_engine, step_fn):
    from aspire_amd.samplers.smc import HipSMC

    lik, prior, _, _, truth = problem_a()
    (z, paths), v = census(hip_engine, lambda: z_scores(hip_engine, HipSMC, lik, prior, D, truth, n_steps=32, step_fn=step_fn))
    assert all("callables: whitened-state session" in p for p in paths), paths
    assert ran(v, "k_fullmixIdLi2ELb0E") > 0 and ran(v, "k_fullmixIdLi2ELb1E") == 0, sorted(v)
    check(z, f"(a) smc {step_fn}")


def test_b_basic_example_uniform_prior(hip_engine):
    from aspire_amd import DiagGaussianMixture, GaussianMixture
    from aspire_amd.samplers.smc import HipSMC

    d = 4
    lik = DiagGaussianMixture(np.full((1, d), 2.0), 1.0)
    prior = GaussianMixture.uniform(-10.0, np.full(d, 10.0))
    (z, paths), v = census(hip_engine, lambda: z_scores(hip_engine, HipSMC, lik, prior, d, -d * math.log(20.0), n_steps=32, step_fn="pcn"))
    assert all("callables" in p for p in paths), paths
    assert ran(v, "k_fullmixIdLi1ELb0E") > 0, sorted(v)
    check(z, "(b) basic example")


def test_c_blackjax_hmc_takes_value_and_gradient_from_the_kernel(hip_engine, monkeypatch):
    from aspire_amd import GaussianMixture
    from aspire_amd.samplers.blackjax_smc import HipBlackJAXSMC

    lik, prior, _, _, truth = problem_a()
    calls = [0]
    plain = GaussianMixture.__call__

    def counted(self, samples):
        calls[0] += 1
        return plain(self, samples)

    monkeypatch.setattr(GaussianMixture, "__call__", counted)
    (z, paths), v = census(hip_engine, lambda: z_scores(hip_engine, HipBlackJAXSMC, lik, prior, D, truth, n=1 << 13, algorithm="hmc",
                                                        step_size=0.15, num_integration_steps=10, n_steps=16))
    assert all("hmc split" in p for p in paths), paths
    assert ran(v, "k_fullmixIdLi2ELb1E") > 0, sorted(v)
    assert calls[0] == 0, f"{calls[0]} torch-ops evaluations of the target"
    check(z, "(c) blackjax_smc hmc")


def test_d_emcee_smc_smoke(hip_engine):
    from aspire_amd.samplers.emcee_smc import HipEmceeSMC

    eng = hip_engine
    lik, prior, _, _, truth = problem_a()
    sp = HipEmceeSMC(log_likelihood=lik, log_prior=prior, dims=D, prior_flow=flow_for(eng, D, 1), xp=np, engine=eng,
                     rng=np.random.default_rng(7))
    out, v = census(eng, lambda: sp.sample(1 << 13, sampler_kwargs=dict(nsteps=20), store_sample_history=False))
    assert "stretch move" in sp.last_mutation_path
    assert ran(v, "k_fullmixIdLi2ELb0E") > 0, sorted(v)
    x = out.x.cpu().numpy() if torch.is_tensor(out.x) else np.asarray(out.x)
    assert np.isfinite(x).all() and np.isfinite(float(out.log_evidence)) and abs(float(out.log_evidence) - truth) < 1.0


def test_d_minipcn_chain_smoke(hip_engine):
    from aspire_amd.samplers.mcmc import HipMiniPCN

    eng = hip_engine
    lik, prior, _, _, _ = problem_a()
    mean, cov = posterior_a()
    n = 2048
    s = HipMiniPCN(log_likelihood=lik, log_prior=prior, dims=D, prior_flow=flow_for(eng, D, 3), xp=np, engine=eng,
                   rng=np.random.default_rng(5))
    out, v = census(eng, lambda: s.sample(n_walkers=n, n_steps=400, last_step_only=True, step_fn="pcn"))
    assert "callables: whitened-state session" in s.last_mutation_path
    assert ran(v, "k_fullmixIdLi2ELb0E") > 0, sorted(v)
    x = out.x.cpu().numpy() if torch.is_tensor(out.x) else np.asarray(out.x)
    assert x.shape == (n, D) and np.isfinite(x).all() and np.isfinite(np.asarray(out.log_likelihood)).all()
    se = np.sqrt(np.diag(cov) / n)  # the walkers are independent chains: the last states are n independent draws
    dev = np.abs(x.mean(axis=0) - mean) / se
    print(f"(d) minipcn: |mean - posterior mean| / standard error = {np.round(dev, 2).tolist()}")
    assert np.all(dev < 5.0), dev
