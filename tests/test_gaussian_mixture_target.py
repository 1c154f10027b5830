"""aspire_amd.GaussianMixture without a GPU: construction, closed forms, the non-finite contract of __call__ on numpy and CPU
torch, autograd against the long-double restatement, the errors it raises, one SMC run through the engine's CPU test double, and
the C ABI's new symbol."""
import math
import os
import re

import numpy as np
import pytest
import torch

import fullmix_ref as R
from aspire_amd import GaussianMixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spd(d, seed, cond=50.0):
    g = np.random.default_rng(seed)
    Q = np.linalg.qr(g.normal(size=(d, d)))[0]
    return (Q * np.geomspace(1.0, cond, d)) @ Q.T


# ---- construction ---------------------------------------------------------------------------------------------------------
def test_covariance_and_precision_construction_agree():
    d, C = 6, 3
    g = np.random.default_rng(0)
    cov = np.stack([spd(d, s) for s in range(C)])
    mu, w = g.normal(size=(C, d)), np.array([1.0, 2.0, 3.0])
    a = GaussianMixture(mu, cov, weights=w)
    b = GaussianMixture(mu, precisions=np.linalg.inv(cov), weights=w)
    x = g.normal(size=(50, d)) * 2
    np.testing.assert_allclose(a(x), b(x), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(a.logw, b.logw, rtol=1e-12)
    for t in (a, b):
        assert t.dims == d and t.n_components == C and t.mu.shape == (C, d) and t.whiten.shape == (C, d, d) and t.logw.shape == (C,)
        assert t.lower is None and t.upper is None
        assert np.all(np.triu(t.whiten, 1) == 0.0)  # lower-triangular
        np.testing.assert_allclose(np.einsum("cki,ckj->cij", t.whiten, t.whiten), np.linalg.inv(cov), rtol=1e-10, atol=1e-12)
    from scipy.stats import multivariate_normal as mvn

    direct = np.log(sum(w[c] / w.sum() * mvn(mu[c], cov[c]).pdf(x) for c in range(C)))
    np.testing.assert_allclose(a(x), direct, rtol=1e-11)


def test_shared_matrix_and_single_mean_broadcast():
    d = 4
    S = spd(d, 3)
    mu = np.random.default_rng(1).normal(size=(3, d))
    a, b = GaussianMixture(mu, S), GaussianMixture(mu, np.tile(S, (3, 1, 1)))
    assert np.array_equal(a.whiten, b.whiten) and np.array_equal(a.logw, b.logw)
    one = GaussianMixture(mu[0], S)
    assert one.n_components == 1 and one.mu.shape == (1, d)
    lo = GaussianMixture(mu, S, bounds=(-1.0, [1.0, 2.0, 3.0, 4.0]))
    assert np.array_equal(lo.lower, -np.ones(d)) and np.array_equal(lo.upper, [1.0, 2.0, 3.0, 4.0])


def test_singular_precisions_are_accepted_and_have_no_constant():
    d = 5
    P = spd(d, 4)
    lam, V = np.linalg.eigh(P)
    lam[0] = 0.0
    Ps = (V * lam) @ V.T
    for prec in (Ps, np.zeros((d, d))):
        t = GaussianMixture(np.zeros(d), precisions=prec, normalized=False)
        np.testing.assert_allclose(t.whiten[0].T @ t.whiten[0], prec, atol=1e-12)
        assert np.all(np.triu(t.whiten[0], 1) == 0.0)
        with pytest.raises(ValueError, match="normalized=False"):
            GaussianMixture(np.zeros(d), precisions=prec)
    x = np.random.default_rng(2).normal(size=(9, d))
    t = GaussianMixture(np.zeros(d), precisions=Ps, normalized=False)
    np.testing.assert_allclose(t(x), -0.5 * np.einsum("ni,ij,nj->n", x, Ps, x), rtol=1e-10, atol=1e-12)


# ---- closed forms ---------------------------------------------------------------------------------------------------------
def test_uniform_is_the_normalised_box():
    lo, hi = np.array([-10.0, 0.0, 2.0]), np.array([10.0, 1.0, 2.5])
    u = GaussianMixture.uniform(lo, hi)
    inside = -float(np.sum(np.log(hi - lo)))
    x = np.array([[0.0, 0.5, 2.25], lo, hi, [10.0, 0.0, 2.5], [np.nextafter(10.0, 11.0), 0.5, 2.25], [0.0, np.nextafter(0.0, -1.0), 2.25],
                  [0.0, 0.5, 2.6]])
    want = np.array([inside] * 4 + [-np.inf] * 3)
    assert np.array_equal(u(x), want) and np.array_equal(u(torch.as_tensor(x)).numpy(), want)
    s = GaussianMixture.uniform(-10.0, [10.0, 10.0])
    assert s.dims == 2 and s(np.zeros((1, 2)))[0] == -2 * math.log(20.0)


@pytest.mark.parametrize("m", [9, 5, 3])
def test_from_linear_model_is_the_direct_evaluation(m):
    d = 5
    g = np.random.default_rng(m)
    A, y, sig = g.normal(size=(m, d)), g.normal(size=m), g.uniform(0.5, 2.0, size=m)
    x = g.normal(size=(40, d)) * 2
    direct = -0.5 * (((y - x @ A.T) / sig) ** 2).sum(axis=1)
    np.testing.assert_allclose(GaussianMixture.from_linear_model(A, y, sig, normalized=False)(x), direct, rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(GaussianMixture.from_linear_model(A, y, sig)(x), direct - np.sum(np.log(sig * math.sqrt(2 * math.pi))),
                               rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(GaussianMixture.from_linear_model(A, y, 0.7, normalized=False)(x),
                               -0.5 * (((y - x @ A.T) / 0.7) ** 2).sum(axis=1), rtol=1e-11, atol=1e-11)


# ---- behaviour ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("namespace", ["numpy", "torch"])
@pytest.mark.parametrize("kind,bounds", [("plain", True), ("flat", False), ("singular", True)])
def test_non_finite_contract(namespace, kind, bounds):
    t, _ = R.make_target(5, 3, 1.0, seed=1, kind=kind, bounds=bounds)
    x = np.concatenate([R.make_rows(t, 20, seed=2), R.special_rows(t)])
    ref = R.reference(t, x)
    got = t(x) if namespace == "numpy" else t(torch.as_tensor(x)).numpy()
    assert np.isnan(ref["value"]).sum() >= 6 and np.isneginf(ref["value"]).sum() >= 6
    wv, _ = R.compare(ref, got)  # the pattern must match exactly; finite rows within the tolerance
    assert wv < 1.0, wv
    with_nan = x[np.isnan(x).any(axis=1)]
    assert np.isnan(t(with_nan)).all()  # NaN wins over +-inf and over the bounds


@pytest.mark.parametrize("d,C,kind", [(3, 1, "plain"), (8, 4, "plain"), (8, 3, "flat"), (33, 2, "singular")])
def test_torch_autograd_matches_the_restatement(d, C, kind):
    t, _ = R.make_target(d, C, 1.0, seed=4, kind=kind, bounds=True)
    x = np.concatenate([R.make_rows(t, 60, seed=5), R.special_rows(t)])
    ref = R.reference(t, x)
    xt = torch.as_tensor(x).requires_grad_(True)
    val = t(xt)
    (g,) = torch.autograd.grad(torch.where(torch.isfinite(val), val, torch.zeros_like(val)).sum(), xt)
    wv, wg = R.compare(ref, val.detach().numpy(), g.numpy())
    assert wv < 1.0 and wg < 1.0, (wv, wg)


def test_value_errors():
    d = 3
    S, mu = spd(d, 0), np.zeros(d)
    with pytest.raises(ValueError, match="exactly one"):
        GaussianMixture(mu)
    with pytest.raises(ValueError, match="exactly one"):
        GaussianMixture(mu, S, precisions=S)
    with pytest.raises(ValueError, match="positive definite"):
        GaussianMixture(mu, np.diag([1.0, -1.0, 1.0]))
    with pytest.raises(ValueError, match="positive definite"):
        GaussianMixture(mu, S + np.triu(np.ones((d, d)), 1))  # not symmetric
    with pytest.raises(ValueError, match="positive definite"):
        GaussianMixture(mu, np.zeros((d, d)))  # semi-definite is not enough for a covariance
    with pytest.raises(ValueError, match="semi-definite"):
        GaussianMixture(mu, precisions=np.diag([1.0, -1e-3, 1.0]), normalized=False)
    with pytest.raises(ValueError, match="symmetric"):
        GaussianMixture(mu, precisions=S + np.triu(np.ones((d, d)), 1))
    with pytest.raises(ValueError, match="normalized=False"):
        GaussianMixture(mu, precisions=np.zeros((d, d)))
    with pytest.raises(ValueError, match="at most 8"):
        GaussianMixture(np.zeros((9, d)), S)
    with pytest.raises(ValueError, match="matrices must be"):
        GaussianMixture(mu, np.eye(4))
    with pytest.raises(ValueError, match="weights"):
        GaussianMixture(np.zeros((2, d)), S, weights=[1.0, -1.0])
    with pytest.raises(ValueError, match="lower <= upper"):
        GaussianMixture(mu, S, bounds=(1.0, 0.0))
    with pytest.raises(ValueError, match="lower < upper"):
        GaussianMixture.uniform(0.0, 0.0)
    with pytest.raises(ValueError, match="sigma positive"):
        GaussianMixture.from_linear_model(np.ones((2, d)), np.zeros(2), 0.0)
    # a rounding-sized negative eigenvalue is accepted
    lam, V = np.linalg.eigh(S)
    lam[0] = -1e-18
    GaussianMixture(mu, precisions=(V * lam) @ V.T, normalized=False)


def test_evaluate_without_a_kernel_is_call(caplog):
    """The engine's CPU test double has no fullmix_logpdf: evaluate is __call__, announced once per instance."""
    import logging

    from oracle_engine import OracleEngine

    t, _ = R.make_target(4, 2, 1.0, seed=0)
    x = torch.as_tensor(R.make_rows(t, 10, seed=0))
    with caplog.at_level(logging.INFO, logger="aspire_amd.targets"):
        a, b = t.evaluate(OracleEngine(), x), t.evaluate(OracleEngine(), x)
        v, g = t.evaluate(OracleEngine(), x, grad=True)
    assert torch.equal(a, t(x)) and torch.equal(a, b) and torch.equal(v, a) and g.shape == x.shape
    assert sum("array ops" in r.message for r in caplog.records) == 1


def test_smc_on_the_test_double_correlated_likelihood_uniform_prior():
    """sample_posterior(sampler="smc") at d = 3: a correlated Gaussian likelihood under GaussianMixture.uniform, through the
    callables path of the engine's CPU double; the evidence is log(1 / 20^3) up to the mass outside the box (< 1e-15)."""
    from aspire_amd import Aspire, Samples
    from oracle_engine import OracleEngine

    d = 3
    params = [f"x_{i}" for i in range(d)]
    cov = spd(d, 7, cond=10.0) / 4.0
    lik = GaussianMixture(np.array([2.0, 1.0, 0.0]), cov)
    prior = GaussianMixture.uniform(-10.0, np.full(d, 10.0))
    eng = OracleEngine()
    g = np.random.default_rng(5)
    train = Samples(g.multivariate_normal([2.0, 1.0, 0.0], cov * 1.5, size=500), parameters=params, xp=np)
    asp = Aspire(log_likelihood=lik, log_prior=prior, dims=d, parameters=params, prior_bounds={p: [-10, 10] for p in params},
                 bounded_to_unbounded=False, flow_backend="gaussian", xp=np, engine=eng, seed=6)
    asp.fit(train)
    out = asp.sample_posterior(n_samples=400, sampler="smc", engine=eng, rng=np.random.default_rng(7))
    assert np.isfinite(float(out.log_evidence)) and np.isfinite(float(out.log_evidence_error))
    assert abs(float(out.log_evidence) + d * math.log(20.0)) < 5 * float(out.log_evidence_error) + 0.1
    assert "callables" in asp.sampler.last_mutation_path
    assert asp.sampler.n_likelihood_evaluations > 0


def test_abi_keeps_its_version_and_gains_the_symbol():
    from aspire_amd import _lib

    header = open(os.path.join(ROOT, "include", "asmc.h")).read()
    assert re.search(r"#define ASMC_ABI_VERSION 33\b", header) and _lib.ASMC_ABI_VERSION == 33
    assert re.search(r"\bint asmc_fullmix_logpdf\(", header) and "asmc_fullmix_logpdf" in _lib.SIGNATURES
    lib = _lib.load()
    assert hasattr(lib, "asmc_fullmix_logpdf") and lib.asmc_abi_version() == 33
    import ctypes

    assert ctypes.sizeof(_lib.AsmcFullMix) == 48 and _lib.AsmcFullMix.logw_dev.offset == 8 and _lib.AsmcFullMix.upper_dev.offset == 40
